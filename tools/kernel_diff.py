"""Are the kernels of two device-only listings the same?  For a change that must not touch device code.
usage: python tools/kernel_diff.py A.s B.s
A listing is `hipcc <build flags minus -fPIC -shared> --cuda-device-only -S offmark_kernels.hip -o A.s` (tools/kernel_resources.py
shows the command), one at each commit.  Kernels are compared per symbol, because their order in the listing follows the order
of instantiation in the host code: the instruction text after removing assembler comments and the function number inside local
labels (.LBB<k>_<i>, .Lfunc_end<k>), and vgpr / sgpr / scratch / LDS from the metadata.  The long-branch labels .Lpost_getpc<j> carry a
serial number that runs through the whole listing, so it moves with the order of the kernels too: they are renumbered inside each
kernel in order of appearance.  For a change that may touch some kernels: every kernel whose text differs is listed with its
instruction line count in A and in B, and the LDS / global / flat atomic instructions are counted per kernel family (the
template's name) in A and in B; every kernel that is only in B is listed with its registers / scratch / LDS and the same three atomic
counts.  Exit status 0 = same set of kernels, all equal."""
import re
import sys

KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    meta = {}
    for b in re.split(r"\n  - \.agpr_count:", text)[1:]:
        get = lambda k: re.search(r"\." + k + r":\s+(\S+)", b).group(1)  # noqa: E731
        meta[get("name")] = tuple(int(get(k)) for k in KEYS)
    body = {}
    for name in meta:
        m = re.search(r"^" + re.escape(name) + r":.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        lines = (re.sub(r"\s*;.*", "", ln).rstrip() for ln in m.group(1).split("\n"))
        code = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end)\d+", r".\1", "\n".join(ln for ln in lines if ln))
        serials = list(dict.fromkeys(re.findall(r"\.Lpost_getpc(\d+)", code)))
        body[name] = re.sub(r"\.Lpost_getpc(\d+)", lambda g: ".Lpost_getpc#%d" % serials.index(g.group(1)), code)
    return meta, body


def family(symbol):
    m = re.match(r"_ZN4ofmk(\d+)", symbol)              # the kernel's name without its template arguments
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


(ma, ba), (mb, bb) = kernels(sys.argv[1]), kernels(sys.argv[2])
only_a, only_b = sorted(set(ma) - set(mb)), sorted(set(mb) - set(ma))
both = sorted(set(ma) & set(mb))
text_differs = [k for k in both if ba[k] != bb[k]]
meta_differs = [k for k in both if ma[k] != mb[k]]
print(f"kernels: {len(ma)} in A, {len(mb)} in B, {len(both)} in both; only in A: {only_a}; only in B: {only_b}")
print(f"instruction text differs: {text_differs}")
print(f"{' / '.join(KEYS)} differ: {[(k, ma[k], mb[k]) for k in meta_differs]}")
print(f"kernels with scratch: {[k for k in mb if mb[k][2]]}")
print(f"instruction lines compared: {sum(b.count(chr(10)) + 1 for b in ba.values())}")
for k in text_differs:
    print(f"  {k}: {ba[k].count(chr(10)) + 1} -> {bb[k].count(chr(10)) + 1} instruction lines")
print("atomic instructions per kernel family (kernels; ds_add / global_atomic / flat_atomic), A -> B:")
for fam in sorted({family(k) for k in both}):
    ks = [k for k in both if family(k) == fam]
    na, nb = ([sum(len(re.findall(r"^\s*" + op, b[k], re.M)) for k in ks) for op in ("ds_add", "global_atomic", "flat_atomic")] for b in (ba, bb))
    if any(na) or any(nb):
        print(f"  {fam} ({len(ks)}): {na[0]} / {na[1]} / {na[2]} -> {nb[0]} / {nb[1]} / {nb[2]}")
if only_b:
    print(f"kernels only in B ({' / '.join(KEYS)}; ds_add / global_atomic / flat_atomic):")
for k in only_b:
    n = [len(re.findall(r"^\s*" + op, bb[k], re.M)) for op in ("ds_add", "global_atomic", "flat_atomic")]
    print(f"  {k}: {' / '.join(map(str, mb[k]))}; {n[0]} / {n[1]} / {n[2]}")
ok = not (only_a or only_b or text_differs or meta_differs)
print("SAME DEVICE CODE" if ok else "DEVICE CODE DIFFERS")
sys.exit(0 if ok else 1)
