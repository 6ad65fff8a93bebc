"""Print per-kernel VGPR / scratch / occupancy of the HIP sources (hipcc -Rpass-analysis), or with
--preload each kernel's kernel-argument preload and what its front still loads, or with --asm-diff REV
whether each source's device assembly equals that of the same file at git revision REV (a refactor's check).

Developer tool, not part of the product package:
`python tools/resource_report.py [--preload | --asm-diff REV] [SRC ...]`."""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zonos_amd.build import ARCH, CSRC, FLAGS, HIPCC  # noqa: E402

KEYS = ("VGPRs", "AGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]")


def report(src: str) -> None:
    r = subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, src),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    cur, info = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur, info = m.group(1), {}
        for key in KEYS:
            m = re.search(key + r": (\d+)", line)
            if m and cur:
                info[key.split(" ")[0].replace("\\", "")] = int(m.group(1))
                if key.startswith("LDS"):
                    flag = " <-- SCRATCH" if info.get("ScratchSize", 0) else ""
                    print(f"{src:12s} {cur[:60]:60s} {info}{flag}")


def device_asm(src: str, csrc: str = CSRC) -> str:
    """The device-only assembly of one source, built with the library's own flags."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc -S failed for {src}:\n{r.stderr}")
        with open(out, encoding="utf-8") as f:
            return f.read()


def kernel_fronts(asm: str) -> dict:
    """Per kernel (mangled name): 'preload' = argument dwords delivered in SGPRs at wave start, 'kernarg' = argument
    bytes, 'front' = the (offset, bytes) of every scalar load from the kernarg pointer (s[0:1] or a plain copy of
    it) between the kernel's real entry -- behind the 256-byte-aligned compatibility prologue a preloading
    kernel starts with -- and its first vector-memory load, 'waited' = those of them that an s_waitcnt lgkmcnt
    waits for before that load: the argument round trips in front of the kernel's data (a load that is only issued
    there returns beside the data loads)."""
    kernels = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        name, body, desc = m.groups()
        pre = int(re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", desc).group(1))
        size = int(re.search(r"\.amdhsa_kernarg_size (\d+)", desc).group(1))
        lines = body.split("\n")
        if pre:
            lines = lines[next(i for i, ln in enumerate(lines) if re.match(r"\s*\.p2align\s+8", ln)):]
        ptrs, front, waited, pending = {"s[0:1]"}, [], [], []
        for ln in lines:
            ln = ln.strip()
            if re.match(r"(global|buffer|flat)_load_", ln):
                break
            c = re.match(r"s_mov_b64 (s\[\d+:\d+\]), (s\[\d+:\d+\])", ln)
            if c and c.group(2) in ptrs:
                ptrs.add(c.group(1))
            ld = re.match(r"s_load_dword(x\d+)? \S+ (s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)", ln)
            if ld and ld.group(2) in ptrs:
                front.append((int(ld.group(3), 0), 4 * int((ld.group(1) or "x1")[1:])))
                pending.append(front[-1])
            if ln.startswith("s_waitcnt") and "lgkmcnt" in ln:
                waited += pending
                pending = []
            # a copy of the pointer ends where its registers are written
            dst = re.match(r"s_\w+ (?:s\[(\d+):(\d+)\]|s(\d+))\b", ln)
            if dst and not (c and c.group(2) in ptrs):
                lo, hi = (int(dst.group(1)), int(dst.group(2))) if dst.group(1) else (int(dst.group(3)),) * 2
                for p in list(ptrs):
                    a, b = map(int, re.findall(r"\d+", p))
                    if a <= hi and lo <= b:
                        ptrs.discard(p)
        kernels[name] = {"preload": pre, "kernarg": size, "front": front, "waited": waited}
    return kernels


def demangle(names) -> dict:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:
        return {n: n for n in names}
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.split("\n") if r.returncode == 0 else list(names)
    return dict(zip(names, out))


def report_preload(src: str) -> None:
    ks = kernel_fronts(device_asm(src))
    nice = demangle(list(ks))
    for name, k in ks.items():
        front = " ".join(f"0x{o:02x}+{n}" + ("(waited)" if (o, n) in k["waited"] else "") for o, n in k["front"]) or "-"
        print(f"{src:12s} {nice[name][:72]:72s} preload {k['preload']:2d} dw of {k['kernarg'] // 4:3d}  front loads {front}")


def kernel_texts(asm: str) -> dict:
    """Per kernel (mangled name): its code and kernel descriptor with the names a renaming changes taken out --
    the kernel's own symbol, the function numbers in local labels, the per-build __hip_cuid_* symbol."""
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n.*?^\s*\.amdhsa_kernel \1\n.*?^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        text = m.group(0).replace(m.group(1), "KERNEL")
        text = re.sub(r"\.L([A-Za-z_]+)\d+", r".L\1", re.sub(r"\bBB\d+_", "BB_", text))
        out[m.group(1)] = re.sub(r"[ \t]+", " ", re.sub(r"__hip_cuid_\w+", "__hip_cuid", text))   # (comment padding)
    return out


def asm_diff(src: str, rev: str) -> bool:
    """Compare src's kernels with those of the same file at `rev` (its whole csrc/ and include/ of that
    revision), as multisets of normalised texts: names may change, code may not."""
    root = os.path.dirname(os.path.dirname(CSRC))
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", root, "archive", rev, "zonos_amd/csrc", "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", d], input=tar.stdout, check=True)
        old = kernel_texts(device_asm(src, os.path.join(d, "zonos_amd", "csrc")))
    new = kernel_texts(device_asm(src))
    nice = demangle(list(new) + list(old))
    left = dict(old)
    for name, text in new.items():
        twin = next((o for o, t in left.items() if t == text), None)
        if twin is not None:
            del left[twin]
            continue
        print(f"{src}: DIFFERS at {nice[name][:100]}")
        if left:
            near = max(left, key=lambda o: difflib.SequenceMatcher(None, left[o], text, autojunk=False).quick_ratio())
            delta = list(difflib.unified_diff(left[near].split("\n"), text.split("\n"), nice[near][:60], "new", n=0, lineterm=""))
            print(f"  nearest of {rev}: {nice[near][:100]} ({len(delta)} diff lines)")
            print("\n".join("  " + ln for ln in delta[:20]))
        return False
    if left:
        print(f"{src}: DIFFERS: {len(left)} kernels of {rev} are gone, first {nice[next(iter(left))][:100]}")
        return False
    print(f"{src}: identical ({len(new)} kernels)")
    return True


def main(argv) -> None:
    if "--asm-diff" in argv:
        i = argv.index("--asm-diff")
        rev, srcs = argv[i + 1], argv[:i] + argv[i + 2:]
        srcs = srcs or sorted(s for s in os.listdir(CSRC) if s.endswith(".hip"))
        sys.exit(0 if all([asm_diff(src, rev) for src in srcs]) else 1)
    preload = "--preload" in argv
    argv = [a for a in argv if a != "--preload"]
    srcs = argv or sorted(s for s in os.listdir(CSRC) if s.endswith(".hip"))
    for src in srcs:
        (report_preload if preload else report)(src)


if __name__ == "__main__":
    main(sys.argv[1:])
