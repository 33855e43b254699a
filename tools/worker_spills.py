"""Where the resident worker's spilled scalar registers are written and read (hipcc -O3 --cuda-device-only -S -gline-tables-only on
gangfit_kernels.hip; compiles only, runs anywhere hipcc does).   python tools/worker_spills.py [extra hipcc flags] > profiles/<tag>_worker_spills.txt
For every instance of fit_worker_kernel: the spilled-SGPR count (the compiler's own remark), the VGPRs whose lanes hold the spills
(the destinations of v_writelane_b32 with a constant lane), the v_writelane / v_readlane on those VGPRs ahead of and behind the kernel's
barrier (behind it = the round loop and the exits), how often each spill lane is written, and the reads per basic block behind the
barrier with the block's first source line (innermost location <- the line of gangfit_worker.inc it was inlined into)."""
import collections, os, re, subprocess, sys, tempfile
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "k8s-spark-scheduler_amd", "csrc")
INC = os.path.join(REPO, "include")
ALGOS = {0: "tightly-pack", 1: "distribute-evenly", 2: "minimal-fragmentation", 3: "az-aware-tightly-pack", 4: "single-az-tightly-pack"}
WRITE = re.compile(r"^\s+v_writelane_b32 (v\d+), s\d+, (\d+)\b")
READ = re.compile(r"^\s+v_readlane_b32 s\d+, (v\d+), (\d+)\b")
LOC = re.compile(r"^\s+\.loc\s.*?;\s*(\S+?):(\d+):\d+(.*)$")
INSN = re.compile(r"^\s+[a-z]\w+")


def compile_asm(extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", INC, "-I", CSRC, "--cuda-device-only", "-S", "-gline-tables-only",
               "-Rpass-analysis=kernel-resource-usage", *extra, os.path.join(CSRC, "gangfit_kernels.hip"), "-o", out]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        with open(out) as f:
            return f.read().split("\n"), err


def remarks(err):  # mangled name -> {sspill, V, scr}
    rows, cur = {}, None
    for line in err.split("\n"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, pat in (("sspill", r"SGPRs Spill: (\d+)"), ("V", r"\bVGPRs: (\d+)"), ("scr", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None and "remark" in line:
                cur[key] = int(m.group(1))
    return rows


def where(loc):  # "innermost file:line <- worker.inc:line" of a .loc comment
    m = LOC.match(loc)
    if not m:
        return "?"
    inner = f"{os.path.basename(m.group(1))}:{m.group(2)}"
    outer = re.findall(r"gangfit_worker\.inc:(\d+):\d+", m.group(3))
    return inner if not outer or inner == f"gangfit_worker.inc:{outer[-1]}" else f"{inner} <- gangfit_worker.inc:{outer[-1]}"


def report(name, body, rem):
    spill_v = sorted({m.group(1) for l in body if (m := WRITE.match(l))}, key=lambda v: int(v[1:]))
    barrier = next((i for i, l in enumerate(body) if re.match(r"^\s+s_barrier\b", l)), len(body))
    writes, reads = [0, 0], [0, 0]
    lane_writes = collections.Counter()
    blocks, cur, last_loc = [], None, ""
    for i, l in enumerate(body):
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            cur = {"label": l.split(":")[0].replace("; %", ""), "reads": 0, "writes": 0, "insns": 0, "loc": "", "named": False, "behind": i > barrier}
            blocks.append(cur)
            continue
        m = LOC.match(l)
        if m:
            if m.group(2) != "0":  # (line 0 = compiler-made code: the block is named by its first real line, else by the last one before it)
                last_loc = l
                if cur is not None and not cur["named"]:
                    cur["loc"], cur["named"] = l, True
            continue
        if not INSN.match(l) or l.lstrip().startswith("."):
            continue
        if cur is not None:
            cur["insns"] += 1
            if not cur["loc"]:
                cur["loc"] = last_loc
        w, r = WRITE.match(l), READ.match(l)
        if w and w.group(1) in spill_v:
            writes[i > barrier] += 1
            lane_writes[(w.group(1), w.group(2))] += 1
            if cur is not None:
                cur["writes"] += 1
        if r and r.group(1) in spill_v:
            reads[i > barrier] += 1
            if cur is not None:
                cur["reads"] += 1
    insns = sum(b["insns"] for b in blocks)
    print(f"## fit_worker_kernel<{name}>: {rem.get('sspill', 0)} spilled SGPRs in {', '.join(spill_v) or 'no VGPR'}; {rem.get('V', 0)} VGPRs, "
          f"scratch {rem.get('scr', 0)}, spilled VGPRs {rem.get('vspill', 0)}; {insns} static instructions in {len(blocks)} blocks")
    print(f"   v_writelane ahead of the barrier {writes[0]:4d}   behind it {writes[1]:4d}")
    print(f"   v_readlane  ahead of the barrier {reads[0]:4d}   behind it {reads[1]:4d}")
    hist = collections.Counter(lane_writes.values())
    print("   spill lanes by number of writes: " + ", ".join(f"{n} x {k} write{'s' if k > 1 else ''}" for k, n in sorted(hist.items())))
    by_line = collections.Counter()
    print("   blocks behind the barrier that touch a spill lane (block, instructions, reads, writes, first source line):")
    for b in blocks:
        if b["behind"] and (b["reads"] or b["writes"]):
            w = where(b["loc"])
            by_line[w.split(" <- ")[-1]] += b["reads"]
            print(f"     {b['label']:12s} {b['insns']:4d} {b['reads']:3d} {b['writes']:3d}  {w}")
    print("   reads behind the barrier by the line of gangfit_worker.inc their block starts at:")
    for w, n in sorted(by_line.items(), key=lambda kv: -kv[1]):
        if n:
            print(f"     {n:4d}  {w}")


if __name__ == "__main__":
    extra = sys.argv[1:]
    lines, err = compile_asm(extra)
    rem = remarks(err)
    print(f"# hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S -gline-tables-only {' '.join(extra)}".rstrip())
    starts = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN7gangfit\S*fit_worker_kernelILi(\d+)E\S*):", l)
        if m:
            starts[int(m.group(2))] = (i, m.group(1))
    for algo in sorted(starts):
        i, mangled = starts[algo]
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        report(ALGOS.get(algo, str(algo)), lines[i:end], rem.get(mangled, {}))
