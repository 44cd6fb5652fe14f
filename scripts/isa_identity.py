"""Are the kernels of two source trees the same machine code? Every .hip of both edyn_amd/csrc directories is compiled for gfx950
with the Makefile's flags to assembly (device code only; no GPU needed); per kernel symbol the instruction text and the kernel
descriptor (.amdhsa_* block: VGPRs, AGPRs, SGPRs, scratch, LDS, kernarg size, ...) are compared. Only what depends on the file a
kernel sits in is ignored: the numbering of local labels and the order of the symbols.
usage: python scripts/isa_identity.py <parent edyn_amd/csrc> [<this tree's edyn_amd/csrc>] [-j N] > profiles/<name>_isa_identity.txt"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only", "-S"]


def assemble(csrc, out, jobs):
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    def one(f):
        subprocess.run(["hipcc", *FLAGS, os.path.join(csrc, f), "-o", os.path.join(out, f[:-4] + ".s")], check=True, capture_output=True)
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, files))
    return files


def normalise(lines):
    text = "\n".join(re.sub(r"\s*;.*$", "", l) for l in lines)   # comments carry label numbers and their column
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", text)
    return text


def kernels(out, files):
    """kernel symbol -> (file, code, descriptor)"""
    found = {}
    for f in files:
        lines = open(os.path.join(out, f[:-4] + ".s")).read().split("\n")
        names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
            d0 = next(i for i in range(a, b) if lines[i].strip() == ".amdhsa_kernel " + name)
            d1 = next(i for i in range(d0, b) if lines[i].strip() == ".end_amdhsa_kernel")
            assert name not in found, name
            found[name] = (f, normalise(lines[a:d0] + lines[d1 + 1:b]), normalise(lines[d0:d1 + 1]))
    return found


def main():
    args = sys.argv[1:]
    jobs = 8   # compilers at a time
    if "-j" in args:
        jobs = int(args[args.index("-j") + 1])
        del args[args.index("-j"):args.index("-j") + 2]
    parent = args[0]
    mine = args[1] if len(args) > 1 else os.path.join(ROOT, "edyn_amd", "csrc")
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ka, kb = kernels(ta, assemble(parent, ta, jobs)), kernels(tb, assemble(mine, tb, jobs))
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    differ = [n for n in sorted(set(ka) & set(kb)) if ka[n][1:] != kb[n][1:]]
    moved = [n for n in sorted(set(ka) & set(kb)) if ka[n][0] != kb[n][0]]
    demangle = lambda n: re.sub(r"\(.*$", "", subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip())
    print("# Kernel-by-kernel comparison of the gfx950 device code of two trees (scripts/isa_identity.py): instruction text and kernel descriptor")
    print(f"kernel symbols, parent: {len(ka)}")
    print(f"kernel symbols, this tree: {len(kb)}")
    print(f"compared: {len(set(ka) & set(kb))}")
    print(f"identical: {len(set(ka) & set(kb)) - len(differ)}")
    print(f"differing: {len(differ)}" + "".join(f"\n  {demangle(n)}" for n in differ))
    print(f"only in the parent: {len(only_a)}" + "".join(f"\n  {demangle(n)}" for n in only_a))
    print(f"only in this tree: {len(only_b)}" + "".join(f"\n  {demangle(n)}" for n in only_b))
    print(f"in another file than in the parent: {len(moved)}")
    for f in sorted({kb[n][0] for n in moved}):
        print(f"  {f}: " + ", ".join(sorted({demangle(n).split('<')[0].replace('void ', '').replace('eh::', '') for n in moved if kb[n][0] == f})))
    return 1 if differ or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main())
