#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same code?

usage: python tools/compare_kernels.py [--rename REGEX REPL]... OLD.so NEW.so [REMOVED_SUBSTRING ...]
(run by path, from any directory; REMOVED_SUBSTRING matches mangled names, so give the length
prefix too: 12k_sgd_chunksI is k_sgd_chunks<...> and not k_sgd_chunks5 or k_sgd_chunks_generic)

--rename pairs a kernel whose template parameters changed with its new name: re.sub(REGEX, REPL)
is applied to every mangled name of OLD before anything is compared, so a renamed kernel is
compared exactly like an unrenamed one.  Two OLD kernels may not end up with one name.

For a change that must not touch device code (a refactor of the host side, a removal of
dead variants): the kernel symbols of NEW must be those of OLD minus the ones containing a
REMOVED_SUBSTRING, and every remaining kernel must keep its registers, LDS, private segment
and its disassembly.  Only what depends on where a kernel sits in its code object is
normalised: the address column and comments, the "..." that objdump prints for zero padding
behind a kernel, and the literal of the s_add_u32 / s_addc_u32 pair that follows an
s_getpc_b64.  Exit status 1 and a list of what differs otherwise."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import code_object_meta as com  # noqa: E402  (tools/ is not a package)

META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


def normalise(text: str) -> list:
    out, pc = [], 0
    for line in text.splitlines():
        s = re.sub(r"^\s*[0-9a-f]+:\s+", "", line.split("//")[0]).strip()
        if not s or s == "...":  # "...": objdump's mark for zero padding behind a kernel
            continue
        if s.startswith("s_getpc_b64"):
            pc = 3  # the two instructions that follow: the s_add_u32 / s_addc_u32 pair
        elif pc and re.match(r"s_addc?_u32 ", s):
            s = re.sub(r",\s*[^,]+$", ", <pc-relative>", s)
        pc = max(pc - 1, 0)
        out.append(s)
    return out


def load(lib: str, renames=()):
    def name(n):
        for pat, repl in renames:
            n = re.sub(pat, repl, n)
        return n

    meta, dis = {}, com.disassembly(lib)
    for k in com.kernels(lib):
        if name(k["name"]) in meta:
            sys.exit(f"--rename gives two kernels one name: {name(k['name'])}")
        meta[name(k["name"])] = tuple(k.get(m) for m in META)
    return meta, {name(n): normalise(t) for n, t in dis.items() if name(n) in meta}


def main() -> int:
    argv, renames = sys.argv[1:], []
    while argv and argv[0] == "--rename":
        renames.append((argv[1], argv[2]))
        argv = argv[3:]
    old_meta, old_dis = load(argv[0], renames)
    new_meta, new_dis = load(argv[1])
    removed = argv[2:]
    gone = set(old_meta) - set(new_meta)
    bad = [f"added: {n}" for n in sorted(set(new_meta) - set(old_meta))]
    bad += [f"missing: {n}" for n in sorted(gone) if not any(r in n for r in removed)]
    for n in sorted(set(old_meta) & set(new_meta)):
        if old_meta[n] != new_meta[n]:
            bad.append(f"metadata {dict(zip(META, old_meta[n]))} -> {new_meta[n]}: {n}")
        if old_dis.get(n) != new_dis.get(n) or not new_dis.get(n):
            bad.append(f"disassembly: {n}")
    per = collections.Counter(r for n in gone for r in removed if r in n)
    print(f"kernels: {len(old_meta)} -> {len(new_meta)}; removed {len(gone)} {dict(per)}; "
          f"{len(set(old_meta) & set(new_meta))} compared, {len(bad)} differences")
    print("\n".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
