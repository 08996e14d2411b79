"""Per-kernel digest of the gfx950 code inside a built library, for comparing the device code of two builds.

    python tools/kernel_digest.py [lib.so]                 one line per kernel: size, VGPRs, private bytes, SHA-256
    python tools/kernel_digest.py new.so --against old.so  the comparison, as markdown (exit 1 on any real difference)

A kernel's digest is the SHA-256 of its disassembly with the instruction encodings (llvm-objdump -d without
addresses), so equal digests mean equal bytes. Moving host code inside a translation unit can move a device global
such as a zero page relative to the kernels that address it pc-relatively; such a kernel differs in the literal of
the s_add_u32 / s_addc_u32 that follows s_getpc_b64 and in nothing else. The comparison accepts exactly that: it
diffs the disassembly without encodings and reports every other changed line as a difference. For each kernel that
is not byte-identical it also says whether the multiset of mnemonics is equal (a different schedule or register
assignment of the same instructions), ignoring the _e32 / _e64 encoding suffix, s_nop and the padding past the last
s_endpgm, and lists the mnemonics whose counts differ. The exit status does not depend on that."""
import argparse
import collections
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scratch_check import LLVM, code_objects, kernel_resources  # noqa: E402

PCREL = re.compile(r"^\s*s_add(c)?_u32 (s\d+), \2, \S+$")


def disassembly(lib, raw, sizes=None):
    """{symbol: [instruction lines]} over the library's gfx950 code objects (sizes: filled with {symbol: bytes})."""
    out = {}
    flags = ["-d", "--no-leading-addr"] + ([] if raw else ["--no-show-raw-insn"])
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(td, "x.so")],
                       check=True, capture_output=True)
        for i, (_, elf) in enumerate(code_objects(open(fat, "rb").read())):
            path = os.path.join(td, f"co{i}.o")
            open(path, "wb").write(elf)
            text = subprocess.run([f"{LLVM}/llvm-objdump", *flags, path], check=True, capture_output=True,
                                  text=True).stdout
            if sizes is not None:
                syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", path], check=True, capture_output=True,
                                      text=True).stdout
                for f in (l.split() for l in syms.splitlines()):  # Num: Value Size Type Bind Vis Ndx Name
                    if len(f) == 8 and f[3] == "FUNC":
                        sizes[f[7]] = int(f[2])
            sym = None
            for line in text.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
                if m:
                    sym = m.group(1)
                    out[sym] = []
                elif sym is not None and line.strip() and line.strip() != "...":  # (... : zero padding past a symbol)
                    out[sym].append(re.sub(r"\s*//.*$", "", line) if not raw else re.sub(r"// [0-9A-F]+:", "//", line))
    return out


def mnemonics(lines):
    """Multiset of a kernel's mnemonics, without the _e32 / _e64 encoding suffix and without s_nop."""
    names = [re.sub(r"_e(32|64)$", "", l.split()[0]) for l in lines]
    while names and names[-1] != "s_endpgm":  # padding past the end disassembles as instructions
        names.pop()
    c = collections.Counter(names)
    del c["s_nop"]
    return c


def digests(lib):
    res = kernel_resources(lib)
    sizes = {}
    dis = disassembly(lib, raw=True, sizes=sizes)
    out = {}
    for kd, (priv, vgprs) in res.items():  # the metadata names the kernel descriptor, <kernel>.kd
        k = kd[:-3] if kd.endswith(".kd") else kd
        out[k] = (sizes[k], vgprs, priv, hashlib.sha256("\n".join(dis[k]).encode()).hexdigest())
    return out


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib", nargs="?", default=os.path.join(here, "distributed-training-comparison_amd", "_lib",
                                                           "libdtc_amd.so"))
    ap.add_argument("--against", default=None)
    a = ap.parse_args()
    new = digests(a.lib)
    if a.against is None:
        for k, (n, vg, priv, h) in sorted(new.items()):
            print(f"{k} bytes={n} vgprs={vg} private={priv} sha256={h}")
        return 0
    old = digests(a.against)
    bad = 0
    print(f"kernel symbols: {len(old)} before, {len(new)} after; added {sorted(set(new) - set(old))}, "
          f"removed {sorted(set(old) - set(new))}\n")
    bad += len(set(new) ^ set(old))
    same = [k for k in new if k in old and new[k] == old[k]]
    print(f"byte-identical: {len(same)} of {len(new)}\n")
    diff = sorted(k for k in new if k in old and new[k] != old[k])
    if diff:
        dn, do = disassembly(a.lib, raw=False), disassembly(a.against, raw=False)
        print("| kernel | code bytes | VGPRs | private B | changed lines | all pc-relative literals | mnemonics |")
        print("|---|---|---|---|---|---|---|")
        moved = {}
        for k in diff:
            mo, mn = mnemonics(do[k]), mnemonics(dn[k])
            moved[k] = [f"{m} {mo[m]} -> {mn[m]}" for m in sorted(set(mo) | set(mn)) if mo[m] != mn[m]]
            res_same = new[k][:3] == old[k][:3]
            lines = [l for l in difflib.unified_diff(do[k], dn[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in
                     ("+++", "---")]
            ok = res_same and len(do[k]) == len(dn[k]) and all(PCREL.match(l[1:]) for l in lines)
            bad += 0 if ok else 1
            print(f"| `{k}` | {old[k][0]} -> {new[k][0]} | {old[k][1]} -> {new[k][1]} | {old[k][2]} -> {new[k][2]} | "
                  f"{len(lines) // 2} | {'yes' if ok else 'NO'} | {'differ' if moved[k] else 'equal'} |")
        for k in diff:
            if moved[k]:
                print(f"\n`{k}` mnemonic counts: " + "; ".join(moved[k]))
    print(f"\nresult: {'equal device code' if bad == 0 else f'{bad} DIFFERENCES'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
