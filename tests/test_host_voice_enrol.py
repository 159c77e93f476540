"""CPU tests of live enrolment: the reserved pool's allocator (RowAllocator: first fit, coalescing, the plans of `compact` and
`extend`, a random run against a brute-force model), holds and the `layout` counter, the default pool unchanged, the argument
refusals of alive_pool_append / alive_pool_move_rows (-1 with a message, nothing launched) and the --pool-rows schedule of the
multistream CLI as pure host logic."""
import ctypes
import random

import pytest
import torch

from module import _native as nat
from module import multistream as MS
from module.multistream import RowAllocator


def _numbers(msg):
    return [int(w.strip(":,.()")) for w in str(msg).split() if w.strip(":,.()").isdigit()]


# ------------------------------------------------------------------------------------------------ the allocator
def test_first_fit_takes_holes_in_address_order_and_the_tail_last():
    a = RowAllocator(100)
    assert [a.add(n, m) for n, m in (("a", 10), ("b", 20), ("c", 10), ("d", 20), ("e", 10))] == [0, 10, 30, 40, 60]
    assert a.holes() == [(70, 30)] and a.free_rows == 30 and a.largest_hole == 30
    a.remove("b")
    a.remove("d")
    assert a.holes() == [(10, 20), (40, 20), (70, 30)]
    assert a.add("f", 15) == 10                       # the first hole that fits, not the best or the largest
    assert a.add("g", 5) == 25                        # what is left of it
    assert a.add("h", 20) == 40                       # the second hole, exactly
    assert a.add("i", 25) == 70                       # only the tail is left
    assert a.holes() == [(95, 5)]
    with pytest.raises(ValueError, match="already in the pool"):
        a.add("a", 1)
    with pytest.raises(ValueError, match="empty"):
        a.add("z", 0)


def test_a_freed_segment_coalesces_with_the_holes_around_it():
    def pool():
        a = RowAllocator(50)
        for n in "abcde":
            a.add(n, 10)
        return a
    a = pool()                                        # a hole before
    a.remove("b")
    a.remove("c")
    assert a.holes() == [(10, 20)] and a.largest_hole == 20 and a.add("x", 20) == 10
    a = pool()                                        # a hole after
    a.remove("c")
    a.remove("b")
    assert a.holes() == [(10, 20)] and a.add("x", 20) == 10
    a = pool()                                        # on both sides
    a.remove("b")
    a.remove("d")
    assert a.holes() == [(10, 10), (30, 10)] and a.largest_hole == 10
    a.remove("c")
    assert a.holes() == [(10, 30)] and a.largest_hole == 30 and a.add("x", 30) == 10
    a = pool()                                        # with the tail
    a.remove("e")
    a.remove("d")
    assert a.holes() == [(30, 20)]
    a = pool()                                        # at the front
    a.remove("a")
    assert a.holes() == [(0, 10)]
    with pytest.raises(ValueError, match="unknown voice"):
        a.remove("a")


def test_add_that_does_not_fit_gives_the_three_numbers_and_changes_nothing():
    a = RowAllocator(100)
    for n, m in (("a", 30), ("b", 20), ("c", 30)):
        a.add(n, m)
    a.remove("b")                                     # holes: 20 at 30, 20 at 80
    before = (dict(a.segments), a.holes(), a.layout)
    with pytest.raises(ValueError) as e:
        a.add("d", 35)
    assert _numbers(e.value)[:4] == [35, 100, 40, 20] and "compact()" in str(e.value)          # needed, capacity, free, largest
    assert (dict(a.segments), a.holes(), a.layout) == before
    with pytest.raises(ValueError) as e:
        a.add("d", 41)
    assert _numbers(e.value)[:4] == [41, 100, 40, 20] and "too small" in str(e.value)
    assert (dict(a.segments), a.holes(), a.layout) == before
    full = RowAllocator(8)                            # a full pool
    full.add("a", 8)
    assert full.free_rows == 0 and full.largest_hole == 0 and full.holes() == []
    with pytest.raises(ValueError) as e:
        full.add("b", 1)
    assert _numbers(e.value)[:4] == [1, 8, 0, 0]
    for bad in (0, -1, 2 ** 31, 1.5, True, None):
        with pytest.raises(ValueError, match="capacity"):
            RowAllocator(bad)
    assert RowAllocator(2 ** 31 - 1).free_rows == 2 ** 31 - 1


def test_compact_plan_is_in_address_order_leaves_no_hole_and_lists_overlapping_moves():
    a = RowAllocator(100)
    for n, m in (("a", 10), ("b", 5), ("c", 30), ("d", 10), ("e", 20)):
        a.add(n, m)
    a.remove("b")                                     # c moves down by 5 < 30: overlapping
    a.remove("d")                                     # e moves down by 15 < 20: overlapping
    moves = a.compact()
    assert moves == [("c", 15, 10, 30), ("e", 55, 40, 20)]
    assert all(src - dst < n for _, src, dst, n in moves)
    assert a.segments == {"a": (0, 10), "c": (10, 30), "e": (40, 20)} and a.holes() == [(60, 40)]
    assert a.compact() == []                          # nothing to move: the layout stays
    # every move's destination is free of OTHER segments' rows at the time it is made
    a = RowAllocator(60)
    for n, m in (("a", 10), ("b", 10), ("c", 10), ("d", 10), ("e", 10)):
        a.add(n, m)
    a.remove("a")
    a.remove("c")
    owner = [None] * 60
    for n, (lo, m) in a.segments.items():
        owner[lo:lo + m] = [n] * m
    for n, src, dst, m in a.compact():
        assert dst < src and all(o in (None, n) for o in owner[dst:dst + m])
        owner[src:src + m] = [None] * m
        owner[dst:dst + m] = [n] * m
    assert owner == ["b"] * 10 + ["d"] * 10 + ["e"] * 10 + [None] * 30


def test_extend_grows_in_place_or_moves_to_a_hole_for_old_and_new_rows():
    a = RowAllocator(100)
    for n, m in (("a", 10), ("b", 10), ("c", 10)):
        a.add(n, m)
    assert a.extend("c", 5) == (20, 10, 20) and a.segments["c"] == (20, 15)         # the tail behind it
    a.remove("b")
    assert a.extend("a", 10) == (0, 10, 0) and a.segments["a"] == (0, 20)           # exactly the hole behind it
    assert a.extend("a", 1) == (0, 20, 35) and a.segments["a"] == (35, 21)          # no room behind: old + new to the tail
    assert a.holes() == [(0, 20), (56, 44)]
    assert a.extend("c", 5) == (20, 15, 0) and a.segments["c"] == (0, 20)           # ... or to an earlier hole that takes both
    before = (dict(a.segments), a.layout)
    with pytest.raises(ValueError) as e:
        a.extend("c", 60)
    assert _numbers(e.value)[-4:] == [80, 100, 59, 44] and (dict(a.segments), a.layout) == before
    with pytest.raises(ValueError, match="unknown voice"):
        a.extend("nobody", 1)
    with pytest.raises(ValueError, match="nothing to append"):
        a.extend("c", 0)


def test_random_operations_against_a_brute_force_model():
    """2 000 operations from a fixed seed; the model is a Python list of the owner of every row"""
    rng = random.Random(20240607)
    cap = 500
    a, owner, nxt = RowAllocator(cap), [None] * 500, 0

    def model_holes():
        out, i = [], 0
        while i < cap:
            if owner[i] is None:
                j = i
                while j < cap and owner[j] is None:
                    j += 1
                out.append((i, j - i))
                i = j
            else:
                i += 1
        return out

    def first_fit(n):
        return next((lo for lo, m in model_holes() if m >= n), None)

    done = {"add": 0, "add-refused": 0, "remove": 0, "extend-in-place": 0, "extend-moved": 0, "extend-refused": 0, "compact": 0}
    for _ in range(2000):
        op = rng.choice(["add", "add", "add", "remove", "remove", "extend", "extend", "compact"])
        names = sorted(a.segments)
        layout = a.layout
        if op == "add":
            n, name = rng.randint(1, 80), f"v{nxt}"
            nxt += 1
            want = first_fit(n)
            if want is None:
                snap = dict(a.segments)
                with pytest.raises(ValueError) as e:
                    a.add(name, n)
                assert _numbers(e.value)[-4:] == [n, cap, owner.count(None), max([m for _, m in model_holes()] or [0])]
                assert a.segments == snap
                done["add-refused"] += 1
            else:
                assert a.add(name, n) == want
                owner[want:want + n] = [name] * n
                done["add"] += 1
            assert a.layout == layout
        elif op == "remove" and names:
            name = rng.choice(names)
            lo, n = a.remove(name)
            assert owner[lo:lo + n] == [name] * n
            owner[lo:lo + n] = [None] * n
            assert a.layout == layout
            done["remove"] += 1
        elif op == "extend" and names:
            name, extra = rng.choice(names), rng.randint(1, 40)
            lo, n = a.segments[name]
            behind = 0
            while lo + n + behind < cap and owner[lo + n + behind] is None:
                behind += 1
            want = lo if behind >= extra else first_fit(n + extra)
            if want is None:
                snap = dict(a.segments)
                with pytest.raises(ValueError):
                    a.extend(name, extra)
                assert a.segments == snap and a.layout == layout
                done["extend-refused"] += 1
            else:
                assert a.extend(name, extra) == (lo, n, want)
                owner[lo:lo + n] = [None] * n
                assert all(o is None for o in owner[want:want + n + extra])
                owner[want:want + n + extra] = [name] * (n + extra)
                assert a.layout == layout + 1
                done["extend-in-place" if want == lo else "extend-moved"] += 1
        elif op == "compact":
            order = [o for i, o in enumerate(owner) if o is not None and (i == 0 or owner[i - 1] != o)]
            moves = a.compact()
            for name, src, dst, n in moves:
                assert dst < src and all(o in (None, name) for o in owner[dst:dst + n])
                owner[src:src + n] = [None] * n
                owner[dst:dst + n] = [name] * n
            assert [o for i, o in enumerate(owner) if o is not None and (i == 0 or owner[i - 1] != o)] == order
            assert len(model_holes()) <= 1 and a.layout == layout + bool(moves)
            done["compact"] += 1
        # after every operation: disjoint segments inside the capacity, the row count, the holes
        mine = [None] * cap
        for name, (lo, n) in a.segments.items():
            assert 0 <= lo and n >= 1 and lo + n <= cap
            assert mine[lo:lo + n] == [None] * n
            mine[lo:lo + n] = [name] * n
        assert mine == owner
        used = sum(n for _, n in a.segments.values())
        assert a.free_rows + used == cap and a.free_rows == owner.count(None)
        assert a.holes() == model_holes()
        assert a.largest_hole == max([m for _, m in model_holes()] or [0])
    assert all(v > 20 for v in done.values()), done         # the run reached every kind of outcome


# ------------------------------------------------------------------------------------------------ holds and layout
def test_a_held_voice_cannot_be_removed_and_layout_counts_only_changes_to_existing_voices():
    a = RowAllocator(100)
    a.add("a", 10)
    a.add("b", 10)
    a.add("c", 10)
    assert a.layout == 0                              # add: no existing voice changed
    a.hold("b", "converter X")
    a.hold("b", "converter X")
    a.hold("b", "converter Y")
    with pytest.raises(ValueError, match="converter X.*converter Y"):
        a.remove("b")
    a.release("b", "converter X")
    a.release("b", "converter Y")
    with pytest.raises(ValueError, match="converter X"):
        a.remove("b")
    assert a.segments["b"] == (10, 10)
    a.release("b", "converter X")
    with pytest.raises(ValueError, match="holds no voice"):
        a.release("b", "converter X")
    with pytest.raises(ValueError, match="unknown voice"):
        a.hold("nobody", "converter X")
    a.remove("b")
    assert a.layout == 0                              # remove: neither
    a.extend("c", 5)
    assert a.layout == 1                              # extend in place: c's length changed
    a.extend("a", 5)
    assert a.layout == 2                              # in place again (b's hole)
    a.extend("a", 10)
    assert a.layout == 3 and a.segments["a"][0] != 0  # moved
    a.compact()
    assert a.layout == 4
    a.compact()
    assert a.layout == 4                              # nothing moved
    a.add("d", 1)
    assert a.layout == 4


# ------------------------------------------------------------------------------------------------ the default pool
def test_default_pool_is_the_class_as_it_stands(monkeypatch):
    """capacity=None: `_tokens` kept, `add` re-packs into a NEW table and bumps `version`; no reserved-pool surface"""
    class FakeLib:
        @staticmethod
        def alive_library_pack_rows(tok, m, d, rows, norms, stream):
            (ctypes.c_float * m).from_address(norms)[:] = [1.0] * m
            return 0
    monkeypatch.setattr(nat, "lib", lambda: FakeLib)
    monkeypatch.setattr(nat, "ptr", lambda t: t.data_ptr())
    monkeypatch.setattr(nat, "stream", lambda: None)
    pool = MS.VoicePool(device="cpu")
    assert pool.capacity is None and pool.version == 0 and pool._tokens == {} and pool.P == 0 and pool.rows is None
    pool.add("a", torch.ones(768, 3))
    rows = pool.rows
    assert pool.version == 1 and list(pool._tokens) == ["a"] and pool.segments == {"a": (0, 3)} and pool.P == 3
    pool.add("b", torch.ones(1, 768, 5))
    assert pool.version == 2 and list(pool._tokens) == ["a", "b"] and pool.segments == {"a": (0, 3), "b": (3, 5)} and pool.P == 8
    assert pool.rows is not rows and pool.rows.shape == (8, 768)
    assert torch.equal(pool.tokens("b"), torch.ones(768, 5))
    for what in ("extend", "remove", "compact"):
        with pytest.raises(ValueError, match="reserved pool"):
            getattr(pool, what)(*(["a", torch.ones(768, 1)] if what == "extend" else ["a"] if what == "remove" else []))
    for what in ("free_rows", "largest_hole", "layout"):
        with pytest.raises(ValueError, match="reserved pool"):
            getattr(pool, what)
    both = MS.VoicePool({"a": torch.ones(768, 2), "b": torch.ones(768, 4)}, device="cpu")
    assert both.version == 1 and both.segments == {"a": (0, 2), "b": (2, 4)}


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_pool_append_and_move_refuse_bad_arguments():
    L = nat.lib()
    ok = dict(tokens=16, rs=10, cs=1, M=10, D=768, rows=16, norms=16, cap=100, at=0, report=16)

    def append(**kw):
        a = dict(ok, **kw)
        return L.alive_pool_append(a["tokens"], a["rs"], a["cs"], a["M"], a["D"], a["rows"], a["norms"], a["cap"], a["at"], a["report"],
                                   None)
    for null in ("tokens", "rows", "norms", "report"):
        assert append(**{null: None}) == -1 and b"null" in L.alive_last_error()
    assert append(D=512) == -1 and b"feature dim 512" in L.alive_last_error()
    assert append(at=91) == -1 and b"[91, +10) outside the table of 100 rows" in L.alive_last_error()       # at + M > capacity
    assert append(at=-1) == -1 and b"outside the table" in L.alive_last_error()
    assert append(M=101) == -1 and b"outside the table" in L.alive_last_error()
    assert append(M=0) == -1
    assert append(at=2 ** 40) == -1 and b"outside the table" in L.alive_last_error()
    assert append(cap=0) == -1 and b"capacity" in L.alive_last_error()
    assert append(cap=2 ** 31) == -1 and b"capacity" in L.alive_last_error()
    assert append(cs=-1) == -1 and b"stride" in L.alive_last_error()

    def move(rows=16, norms=16, cap=100, src=0, dst=50, n=10):
        return L.alive_pool_move_rows(rows, norms, cap, src, dst, n, None)
    assert move(rows=None) == -1 and b"null" in L.alive_last_error()
    assert move(norms=None) == -1 and b"null" in L.alive_last_error()
    assert move(rows=12) == -1 and b"aligned" in L.alive_last_error()
    assert move(src=91) == -1 and b"10 rows from 91 to 50 outside the table of 100 rows" in L.alive_last_error()
    assert move(dst=91) == -1 and b"outside the table" in L.alive_last_error()
    assert move(src=-1) == -1 and move(dst=-1) == -1 and move(n=0) == -1 and move(n=101) == -1
    assert move(cap=2 ** 31) == -1 and b"capacity" in L.alive_last_error()
    assert move(src=20, dst=20) == 0                  # nothing to move: nothing launched


# ------------------------------------------------------------------------------------------------ the CLI's schedule
def test_pool_rows_plan_enrols_at_first_need_and_removes_after_the_last_user():
    import multistream_inference as cli
    sessions = [dict(start=0, ticks=6, voices={"a": 100}),                       # ticks 0..5
                dict(start=2, ticks=2, voices={"b": 50}),                        # ticks 2..3
                dict(start=3, ticks=5, voices={"a": 100, "c": 30}),              # a blend, ticks 3..7: a lives on past session 0
                dict(start=4, ticks=0, voices={"never": 1000}),                  # no whole chunk: never opens
                dict(start=6, ticks=3, voices={"b": 50}),                        # b again after it was removed, ticks 6..8
                dict(start=8, ticks=1, voices={"d": 60})]                        # opens and closes in tick 8
    events, peak = cli.enrol_plan(sessions)
    assert events == [(0, "enrol", "a"), (2, "enrol", "b"), (3, "enrol", "c"), (3, "remove", "b"), (6, "enrol", "b"),
                      (7, "remove", "a"), (7, "remove", "c"), (8, "enrol", "d"), (8, "remove", "b"), (8, "remove", "d")]
    assert peak == 180                                # tick 3: a + b + c (b goes after the tick's step); 6-7: a + c + b
    assert sum(m for s in sessions if s["ticks"] for m in set(s["voices"].values())) > peak
    # shared voices are enrolled once and removed after the last user
    events, peak = cli.enrol_plan([dict(start=0, ticks=3, voices={"a": 10}), dict(start=1, ticks=5, voices={"a": 10})])
    assert events == [(0, "enrol", "a"), (5, "remove", "a")] and peak == 10
    with pytest.raises(ValueError, match="10 and 11 rows"):
        cli.enrol_plan([dict(start=0, ticks=3, voices={"a": 10}), dict(start=1, ticks=5, voices={"a": 11})])
    assert cli.enrol_plan([dict(start=0, ticks=0, voices={"a": 10})]) == ([], 0)
    args = cli.build_parser().parse_args(["s.json", "--pool-rows", "1234"])
    assert args.pool_rows == 1234 and cli.build_parser().parse_args(["s.json"]).pool_rows is None


def test_run_calls_its_hooks_around_every_tick():
    import numpy as np
    import multistream_inference as cli
    log = []

    class Conv:
        def open(self, i, **p):
            log.append(("open", i))

        def step(self, feed):
            log.append(("step", sorted(feed)))
            return {i: None for i in feed}

        def close(self, i):
            log.append(("close", i))
    cli.run(Conv(), [np.zeros(8, np.int16)], [1], 4, [{}], before=lambda t: log.append(("before", t)),
            after=lambda t: log.append(("after", t)))
    assert log == [("before", 0), ("step", []), ("after", 0), ("before", 1), ("open", 0), ("step", [0]), ("after", 1),
                   ("before", 2), ("step", [0]), ("close", 0), ("after", 2)]
