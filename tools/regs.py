"""Register / scratch / occupancy table of the kernels in one csrc/*.hip (cross-compiled to gfx950 assembly with the
Makefile's flags for that file).  usage: python tools/regs.py nnconv_mfma [--against OTHER_CSRC] [extra hipcc flags]
--against: the same file of a second csrc directory (e.g. a checkout of the parent commit) is compiled too and every kernel
is compared with its namesake: resources of both, opcode histograms equal or not, listings equal or not (comments,
compilation-unit ids and the function numbers inside local labels stripped)."""
import collections, re, subprocess, sys, os
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
other = args.pop(args.index("--against") + 1) if "--against" in args else None
if other:
    args.remove("--against")
name, extra = args[0], args[1:]
KEYS = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"),
        ("occ", "Occupancy"))


def kernels(src, out):
    """{symbol: (resource figures, opcode histogram, stripped listing)} of src/name.hip, assembly left in `out`"""
    var = dict(re.findall(r"^(\w+)\s*=\s*(.*)$", open(os.path.join(src, "Makefile")).read(), re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var.get("FLAGS_" + name, ""))
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{root}/include", f"-I{src}", "-Wno-unused-result",
           "-Wno-pass-failed", "-S", "--cuda-device-only", "-o", out, os.path.join(src, name + ".hip")] + flags.split() + extra
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    res = {}
    for f in re.split(r"\n(?=_Z\w+:)", open(out).read()):
        m = re.match(r"(_Z\w+):", f)
        if not m or "NumVgprs" not in f:
            continue
        body = re.sub(r"__hip_cuid_\w+", "", re.sub(r"\.L(\w+?)\d+_", r".L\1_", f.split(".Lfunc_end")[0]))
        lines = [s for s in (re.sub(r"\s*;.*", "", ln).rstrip() for ln in body.split("\n")[1:]) if s]
        ops = collections.Counter(s.split()[0] for s in lines if s[0] in " \t" and s.split()[0][0] != ".")
        res[m.group(1)] = ({k: re.search(r"; %s: (\d+)" % key, f).group(1) for k, key in KEYS}, ops, lines)
    return res


def demangled(sym):
    return subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().split("(")[0][:70]


new = kernels(os.path.join(root, "gnn_qot_estimation_amd", "csrc"), f"/tmp/{name}.s")
if not other:
    for sym, (fig, ops, _) in new.items():
        print(f"{demangled(sym):70s} vgpr {fig['vgpr']:>3s} agpr {fig['agpr']:>3s} scratch {fig['scratch']:>4s} occ {fig['occ']}"
              f" mfma {sum(n for o, n in ops.items() if o.startswith('v_mfma'))}")
else:
    old = kernels(other, f"/tmp/{name}.against.s")
    # namesakes by demangled name without the argument list: a kernel that gained an argument is still compared with itself
    new, old = ({demangled(sym): v for sym, v in d.items()} for d in (new, old))
    for sym in sorted(set(new) | set(old)):
        if sym not in new or sym not in old:
            print(f"{sym:70s} only in the {'first' if sym in new else 'second'} build")
            continue
        (fn, on, ln), (fo, oo, lo) = new[sym], old[sym]
        diff = {o: on[o] - oo[o] for o in set(on) | set(oo) if on[o] != oo[o]}
        print(f"{sym:70s} " + " ".join(f"{k} {fn[k]}/{fo[k]}" for k, _ in KEYS) +
              f" | figures {'equal' if fn == fo else 'DIFFER'} | opcodes {'equal' if not diff else 'DIFFER ' + str(diff)}"
              f" | listing {'identical' if ln == lo else 'differs'}")
print("asm:", f"/tmp/{name}.s")
