"""Compare the gfx950 kernels of two fat objects (a refactor's before / after).  No GPU needed.
    python tools/cmp_kernels.py OLD.o NEW.o [NAME_SUBSTRING | OLD_SUBSTRING=NEW_SUBSTRING ...]
Per kernel whose mangled name contains one of the substrings (every kernel without one): "same sequence" (the disassembly agrees
instruction for instruction, operands included), "same multiset" (the same opcodes as often, in another order or with other
registers) or "differs" (with the opcodes whose counts moved), and the resource numbers of tools/kernel_resources.py where they
moved.  Kernels are matched by demangled name with the namespace qualifiers dropped (a type that moved into a header keeps its
kernel); two kernels of one object that differ by namespace only are an error.  A renamed kernel is paired by hand:
OLD_SUBSTRING=NEW_SUBSTRING pairs the one kernel of OLD.o whose demangled name contains the left side with the one of NEW.o whose
name contains the right side; the pairs are taken in order, and a side must select exactly one kernel among those not paired yet.
Exit status 1 when a kernel differs, its resources moved, or it exists on one side only.  The row write of csrc/prefill.hip, three
kernels before it became one template:
    python tools/cmp_kernels.py OLD/prefill.o NEW/prefill.o 'rope_cache_rows_kv8_kernel<false, false>=rope_cache_rows_kernel<false, false, true>' \
        'rope_cache_rows_kv8_kernel<true, false>=rope_cache_rows_kernel<true, false, true>' \
        'rope_cache_rows_kv8_kernel<false, true>=rope_cache_rows_kernel<false, true, true>' \
        'qknorm_rope_cache_rows_kernel(=rope_cache_rows_kernel<true, false, false>' 'rope_cache_rows_kernel(=rope_cache_rows_kernel<false, false, false>'"""
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
    old, new = argv[0], argv[1]
    subs, pairs = [a for a in argv[2:] if "=" not in a], [a.split("=", 1) for a in argv[2:] if "=" in a]
    res, ins = [], []
    for o in (old, new):
        ks = kernels_of(o)
        keys = [re.sub(r"(\(anonymous namespace\)|\w+)::", "", d) for d in demangle([k[0] for k in ks])]
        # (a kernel named by a pair is compared whatever the name filters say)
        keep = [not subs or any(s in k[0] for s in subs) or any(side in key for pair in pairs for side in pair) for k, key in zip(ks, keys)]
        ks, keys = [k for k, y in zip(ks, keep) if y], [key for key, y in zip(keys, keep) if y]
        code = instructions_of(o, [k[0] for k in ks])
        if len(set(keys)) != len(keys):
            sys.exit(f"{o}: kernels that differ by namespace only: {sorted(k for k in set(keys) if keys.count(k) > 1)}")
        res.append({key: k[1:] for key, k in zip(keys, ks)})
        ins.append({key: code[k[0]] for key, k in zip(keys, ks)})
    shown = {}  # the key of a hand-paired kernel -> its two names
    for a, b in pairs:
        hit = [[k for k in res[i] if sub in k and k not in shown] for i, sub in enumerate((a, b))]
        if len(hit[0]) != 1 or len(hit[1]) != 1:
            sys.exit(f"{a}={b}: the sides select {len(hit[0])} and {len(hit[1])} unpaired kernels, not one each")
        k0, k1 = hit[0][0], hit[1][0]
        if k0 != k1:
            if k1 in res[0]:
                sys.exit(f"{a}={b}: OLD has a kernel of the new name too")
            res[0][k1], ins[0][k1] = res[0].pop(k0), ins[0].pop(k0)
        shown[k1] = f"{k0.split('(')[0]} => {k1}"
    bad = 0
    tally = collections.Counter()
    for n in sorted(set(res[0]) | set(res[1])):
        pretty = shown.get(n, n)
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
