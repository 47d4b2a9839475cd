"""Do two source trees compile to the same device code?  For a refactor that must not change a shipped kernel.

    python karanta_ocr_amd/csrc/tools/device_code_diff.py ROOT_A kr_attention.hip,kr_attn_decode.hip ROOT_B kr_attention.hip,kr_attn_decode.hip

ROOT_* are checkouts of this repository; the files are names under karanta_ocr_amd/csrc/ of each.  Every file is compiled with
the build's flags to device assembly, the kernels of a root's files are pooled by symbol (a kernel may move between files),
comments are dropped and the numbered local labels normalised, and the texts are compared for equality: per symbol `same`,
`differs`, `only in A` or `only in B`.  Exit status 1 if any kernel differs.  CPU only.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..")))
from karanta_ocr_amd import build as B  # noqa: E402


def kernels(root, files, tmp):
    """{kernel symbol: its instruction text + its .amdhsa_kernel block} over the files of one root."""
    out = {}
    flags = [f for f in B.FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S"]
    for i, f in enumerate(files):
        asm = os.path.join(tmp, f"{i}.s")
        subprocess.check_call([B._hipcc(), *flags, os.path.join(root, "karanta_ocr_amd", "csrc", f), "-o", asm])
        text = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", open(asm).read()))
        text = "\n".join(ln for ln in text.split("\n") if ln.strip())
        for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
            s = re.escape(sym)
            body = re.search(rf"^{s}:\n.*?(?=^\.Lfunc_end\d+:$)", text, re.M | re.S).group(0)
            desc = re.search(rf"^\s*\.amdhsa_kernel {s}\n.*?^\s*\.end_amdhsa_kernel$", text, re.M | re.S).group(0)
            out[sym] = body + "\n" + desc
    return out


def main():
    root_a, files_a, root_b, files_b = sys.argv[1], sys.argv[2].split(","), sys.argv[3], sys.argv[4].split(",")
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = kernels(root_a, files_a, ta), kernels(root_b, files_b, tb)
    demangle = subprocess.run(["c++filt"], input="\n".join(sorted(set(a) | set(b))), capture_output=True, text=True).stdout.split("\n")
    bad = 0
    for sym, name in zip(sorted(set(a) | set(b)), demangle):
        verdict = "only in A" if sym not in b else "only in B" if sym not in a else "same" if a[sym] == b[sym] else "differs"
        bad += verdict == "differs"
        print(f"{verdict:10s} {name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
