"""do two gfx950 listings hold the same kernels?  python tools/same_kernels.py parent.s new.s
Compares per kernel, not per file: implicit instantiations are emitted in the order the host code first names them, and local labels
carry the function's ordinal (.LBB<ordinal>_<block>).  Comments and that ordinal are dropped; every kernel symbol (.amdhsa_kernel) must
exist on both sides with equal instruction text.  Exit status 0 = same device code: the check of a host-only change.  Listings:
hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o x.s, both from the same path."""
import re, sys


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = text[text.index(f"\n{name}:") + 1:]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        lines = (re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", ln.split(";")[0]).rstrip() for ln in body.splitlines())
        out[name] = "\n".join(ln for ln in lines if ln.strip())
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
print(f"{len(a)} kernels / {len(b)} kernels, {len(a.keys() ^ b.keys())} on one side only, {len(differ)} bodies differ")
for k in sorted(a.keys() ^ b.keys()) + differ:
    print("  ", k)
sys.exit(1 if a.keys() ^ b.keys() or differ else 0)
