"""Compare the gfx950 kernels of two fat objects (a refactor's before / after).  No GPU needed.
    python tools/cmp_kernels.py OLD.o NEW.o [NAME_SUBSTRING ...]
Per kernel whose mangled name contains one of the substrings (every kernel without one): "same sequence" (the disassembly agrees
instruction for instruction, operands included), "same multiset" (the same opcodes as often, in another order or with other
registers) or "differs" (with the opcodes whose counts moved), and the resource numbers of tools/kernel_resources.py where they
moved.  Kernels are matched by demangled name with the namespace qualifiers dropped (a type that moved into a header keeps its
kernel); two kernels of one object that differ by namespace only are an error.  Exit status 1 when a kernel differs, its resources
moved, or it exists on one side only."""
import collections, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import BIN, demangle, kernels_of  # noqa: E402


def instructions_of(obj, names):
    """{mangled name: [(opcode, operands)]} of the kernels of one fat object"""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        subprocess.check_call([f"{BIN}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull])
        subprocess.check_call([f"{BIN}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        out = {}
        for n in names:
            text = subprocess.run([f"{BIN}/llvm-objdump", "-d", co, f"--disassemble-symbols={n}"], capture_output=True, text=True, check=True).stdout
            ins = []
            for line in text.split("\n"):
                m = re.match(r"\s+(\S+)\s*(.*?)\s*//", line)  # (instruction lines carry their address and encoding in a comment)
                if m:
                    ins.append((m.group(1), m.group(2)))
            out[n] = ins
    return out


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    old, new, subs = argv[0], argv[1], argv[2:]
    res, ins = [], []
    for o in (old, new):
        ks = [k for k in kernels_of(o) if not subs or any(s in k[0] for s in subs)]
        code = instructions_of(o, [k[0] for k in ks])
        keys = [re.sub(r"(\(anonymous namespace\)|\w+)::", "", d) for d in demangle([k[0] for k in ks])]
        if len(set(keys)) != len(keys):
            sys.exit(f"{o}: kernels that differ by namespace only: {sorted(k for k in set(keys) if keys.count(k) > 1)}")
        res.append({key: k[1:] for key, k in zip(keys, ks)})
        ins.append({key: code[k[0]] for key, k in zip(keys, ks)})
    bad = 0
    tally = collections.Counter()
    for n in sorted(set(res[0]) | set(res[1])):
        pretty = n
        if n not in res[0] or n not in res[1]:
            print(f"only in {'OLD' if n in res[0] else 'NEW'}  {pretty[:140]}")
            bad += 1
            continue
        a, b = ins[0][n], ins[1][n]
        ca, cb = collections.Counter(i[0] for i in a), collections.Counter(i[0] for i in b)
        if a == b:
            verdict = "same sequence"
        elif ca == cb:
            verdict = "same multiset"
        else:
            moved = " ".join(f"{op}:{ca[op]}->{cb[op]}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op])
            verdict = f"differs ({len(a)} -> {len(b)} instructions; {moved})"
            bad += 1
        tally[verdict.split(" (")[0]] += 1
        r = "v=%d a=%d s=%d vspill=%d sspill=%d scratch=%d lds=%d" % res[1][n]
        if res[0][n] != res[1][n]:
            r = "RESOURCES MOVED: " + "v=%d a=%d s=%d vspill=%d sspill=%d scratch=%d lds=%d" % res[0][n] + " -> " + r
            bad += 1
        print(f"{verdict:14s} n={len(b):5d} {r}  {pretty[:140]}")
    print(", ".join(f"{v} {k}" for k, v in sorted(tally.items())) + f"; {bad} findings")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
