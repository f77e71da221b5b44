#!/usr/bin/env python3
"""Turn the raw output of tools/refresh_profiles.sh (gpurun_out/<tag>f) into the committed summaries under profiles/.
usage: python tools/make_profiles.py gpurun_out/r02f r02"""
import csv, glob, json, os, re, shutil, sys
from collections import defaultdict
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else "gpurun_out/r03f")
tag = sys.argv[2] if len(sys.argv) > 2 else "r03"
sys.path.insert(0, ROOT)
from bench import kernel_source_hash as _local_hash
out = os.path.join(ROOT, "profiles")
_hp = os.path.join(src, "source_hash.txt")
_measured = open(_hp).read().strip() if os.path.exists(_hp) else None
if _measured and _measured != _local_hash():
    print(f"WARNING: the raw data was measured on kernel sources {_measured}, the tree is now {_local_hash()}")


def kernel_source_hash():
    """the hash of the sources the raw data was MEASURED on (written on the GPU box), else of the local tree"""
    return _measured or _local_hash()


line = json.load(open(os.path.join(src, "bench_line.json")))
json.dump(line, open(os.path.join(out, f"{tag}_bench_line.json"), "w"), indent=1)
stats_line = json.load(open(os.path.join(src, "stats_line.json")))

stats = max(glob.glob(os.path.join(src, "stats/*/*kernel_stats.csv")), key=os.path.getmtime)   # newest run
shutil.copy(stats, os.path.join(out, f"{tag}_bench_kernel_stats.csv"))
rows = list(csv.DictReader(open(stats)))
fwd_k = ("hashgrid_fwd", "untranspose_feats", "psort_")
with open(os.path.join(out, f"{tag}_bench_rocprof_summary.md"), "w") as f:
    f.write("# rocprofv3 --kernel-trace --stats -- python3 bench.py --steps 30 --warmup 5 --no-cpu-baseline "
            "--psnr-steps 0 --nerf-steps 0 --no-secondary\n\n")
    f.write(f"Workload S1 (3-D nerf_hash grid L16 F2 bw19, N = 2^20 per step), MI355X, {tag} (final kernels, source hash "
            f"{kernel_source_hash()}). 35 calls = 5 warm-up + 30 timed.\n")
    f.write(f"bench.py's own HIP-event timing in the same run: forward {stats_line['ms']['forward']:.3f} ms, backward "
            f"{stats_line['ms']['backward']:.3f} ms per step ({stats_line['value'] / 1e6:.0f} M samples/s).\n\n")
    f.write("| kernel | calls | avg us | % |\n|---|---|---|---|\n")
    tf = tb = 0.0
    for r in rows:
        if int(r["Calls"]) < 30 and "rocclr" not in r["Name"]:
            continue
        avg = float(r["AverageNs"]) / 1e3
        f.write(f"| `{r['Name'][:90]}` | {r['Calls']} | {avg:.1f} | {float(r['Percentage']):.2f} |\n")
        per_step = float(r["TotalDurationNs"]) / 35 / 1e3
        if any(k in r["Name"] for k in fwd_k):
            tf += per_step
        elif "shacira::" in r["Name"] or "fillBuffer" in r["Name"]:
            tb += per_step
    f.write(f"\nforward operator = sample sort (psort_partition + psort_local: the batch's plan) + "
            f"hashgrid_fwd_level_pair (fine levels) + hashgrid_fwd_rows (coarse levels + row assembly) = {tf:.1f} us of kernel "
            f"time; backward operator (planned: sorted order) = zero_unowned_rows + front16<SORTED> (gradient rows gathered in plan "
            f"order, 16-byte transpose + bucket counts) + bin_scan_buckets + bin_scatter + bin_consume with brick_accumulate "
            f"(dense coarse levels) on the side stream beside it = {tb:.1f} us of kernel time per step -- a SUM of durations: the "
            f"brick pass overlaps the consume pass, so the operator's wall time is shorter (DESIGN.md 4.3).\n")

def counter(dirname):
    f = max(glob.glob(os.path.join(src, dirname, "*/*counter_collection.csv")), key=os.path.getmtime)
    acc, calls = defaultdict(float), defaultdict(int)
    for r in csv.DictReader(open(f)):
        name = re.sub(r"^void ", "", r["Kernel_Name"]).split("(")[0]
        acc[name] += float(r["Counter_Value"])
        calls[name] += 1
    return acc, calls

ops = {}
fe, calls = counter("pmc_pair_FETCH_SIZE")
wr, _ = counter("pmc_pair_WRITE_SIZE")
iters = 3
for key in ("forward", "backward"):
    kern = {}
    rd = wt = 0.0
    for name in fe:
        if "shacira::" not in name:
            continue
        is_fwd = any(k in name for k in fwd_k)
        if is_fwd != (key == "forward"):
            continue
        kern[name] = {"FETCH_SIZE_KiB_raw": fe[name] / iters, "WRITE_SIZE_KiB_raw": wr.get(name, 0.0) / iters}
        rd += 2 * fe[name] / iters * 1024
        wt += wr.get(name, 0.0) / iters * 1024
    ops[key] = {"read_bytes_corrected": rd, "write_bytes": wt, "hbm_bytes_per_launch": rd + wt, "kernels": kern}
json.dump({"kernel_source_hash": kernel_source_hash(),
           "note": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in SEPARATE passes over `python3 tools/plan_prof.py 3` "
                   "(the PLANNED operator pair of bench.py's step on workload S1: 3-D L16 F2 bw19, N=2^20; 3 calls, per-call "
                   "averages; kernels attributed to forward / backward by name). Counters are in "
                   "KiB; on gfx950 FETCH_SIZE counts 128-B requests as 64 B (MI355X_MICROARCH.md, HBM section), so read "
                   "bytes = 2*FETCH_SIZE*1024 (verified: the transposes read 128 MiB and report 64 MiB); WRITE_SIZE is "
                   "exact.",
           "operators": ops}, open(os.path.join(out, f"{tag}_pmc_traffic.json"), "w"), indent=1)
for k, v in ops.items():
    print(k, "HBM bytes per launch %.3f GB (read %.3f, write %.3f)" % (v["hbm_bytes_per_launch"] / 1e9, v["read_bytes_corrected"] / 1e9, v["write_bytes"] / 1e9))

# extra summaries of this round
for name in ("parity_and_timing.txt", "config_c.txt", "tiled_check.txt"):
    p = os.path.join(src, name)
    if os.path.exists(p):
        shutil.copy(p, os.path.join(out, f"{tag}_{name}"))

# forward unit counters (judge r1 item 3): per kernel, per call
def ctr(dirname):
    fs = glob.glob(os.path.join(src, dirname, "*/*counter_collection.csv"))
    if not fs:
        return {}
    acc, n = defaultdict(lambda: defaultdict(float)), defaultdict(lambda: defaultdict(int))
    for r in csv.DictReader(open(max(fs, key=os.path.getmtime))):
        name = re.sub(r"^void ", "", r["Kernel_Name"]).split("(")[0]
        acc[name][r["Counter_Name"]] += float(r["Counter_Value"])
        n[name][r["Counter_Name"]] += 1
    return {k: {c: v / n[k][c] for c, v in d.items()} for k, d in acc.items()}

with open(os.path.join(out, f"{tag}_fwd_counters.md"), "w") as f:
    f.write(f"# Forward kernels on S1 (N = 2^20), unit counters per launch ({tag}, source hash {kernel_source_hash()})\n\n"
            "`rocprofv3 --pmc <group> --kernel-trace -- python3 tools/fwd_only.py fwd -1 3 3`, one pass per counter group "
            "(SQ / TA / TCP / TCC), averages over 3 calls. `tiled` = cell-sorted path (default), `plain` = "
            "SHACIRA_OPTIONS=tiled=0 (level-per-XCD pair kernel over all 16 levels + untranspose).\n")
    for mode in ("tiled", "plain"):
        merged = defaultdict(dict)
        for grp in ("sq", "ta", "tcp", "tcc"):
            for k, d in ctr(f"ctr_{mode}_{grp}").items():
                if "shacira::" in k:
                    merged[k].update(d)
        f.write(f"\n## {mode}\n\n")
        for k, d in merged.items():
            f.write(f"### `{k}`\n\n| counter | per launch |\n|---|---|\n")
            for c in sorted(d):
                f.write(f"| {c} | {d[c]:,.0f} |\n")
            gui = d.get("GRBM_GUI_ACTIVE"); ta = d.get("TA_TA_BUSY_sum"); hit = d.get("TCC_HIT_sum"); miss = d.get("TCC_MISS_sum")
            notes = []
            if gui and ta:
                notes.append(f"TA busy = TA_TA_BUSY_sum / (256 TAs x GRBM_GUI_ACTIVE / 8 XCDs) = {ta / (256 * gui / 8):.2f}")
            if hit is not None and miss is not None and hit + miss > 0:
                notes.append(f"L2 hit rate = {hit / (hit + miss):.3f}")
            if d.get("SQ_WAVE_CYCLES"):
                notes.append(f"waves parked in waits = SQ_WAIT_ANY / SQ_WAVE_CYCLES = {d.get('SQ_WAIT_ANY', 0) / d['SQ_WAVE_CYCLES']:.2f}")
            if d.get("SQ_WAVES") and d.get("SQ_INSTS_VALU"):
                notes.append(f"VALU instructions per wave = {d['SQ_INSTS_VALU'] / d['SQ_WAVES']:.0f}, VMEM reads per wave = {d.get('SQ_INSTS_VMEM_RD', 0) / d['SQ_WAVES']:.1f}")
            f.write("\n" + "; ".join(notes) + "\n\n")
print("wrote", f"{tag}_fwd_counters.md")


# backward unit counters (round 3)
with open(os.path.join(out, f"{tag}_bwd_counters.md"), "w") as f:
    f.write(f"# Backward kernels on S1 (N = 2^20), unit counters per launch ({tag}, source hash {kernel_source_hash()})\n\n"
            "`rocprofv3 --pmc <group> --kernel-trace -- python3 tools/plan_prof.py 3` (the planned pair; backward kernels listed), one pass per counter group "
            "(SQ / LDS / TCC), averages over 3 calls.\n\n")
    merged = defaultdict(dict)
    for grp in ("sq", "lds", "tcc"):
        for k, d in ctr(f"ctr_bwd_{grp}").items():
            if "shacira::" in k and not any(fk in k for fk in fwd_k):
                merged[k].update(d)
    for k, d in merged.items():
        f.write(f"### `{k}`\n\n| counter | per launch |\n|---|---|\n")
        for c in sorted(d):
            f.write(f"| {c} | {d[c]:,.0f} |\n")
        notes = []
        if d.get("SQ_WAVE_CYCLES"):
            notes.append(f"waves parked in waits = SQ_WAIT_ANY / SQ_WAVE_CYCLES = {d.get('SQ_WAIT_ANY', 0) / d['SQ_WAVE_CYCLES']:.2f}")
        if d.get("SQ_WAVES") and d.get("SQ_INSTS_VALU"):
            notes.append(f"VALU instructions per wave = {d['SQ_INSTS_VALU'] / d['SQ_WAVES']:.0f}, LDS instructions per wave = {d.get('SQ_INSTS_LDS', 0) / d['SQ_WAVES']:.0f}")
        if d.get("SQ_LDS_IDX_ACTIVE") and d.get("SQ_BUSY_CYCLES"):
            notes.append(f"LDS bank-conflict share of LDS-active cycles = {d.get('SQ_LDS_BANK_CONFLICT', 0) / d['SQ_LDS_IDX_ACTIVE']:.2f}")
        hit, miss = d.get("TCC_HIT_sum"), d.get("TCC_MISS_sum")
        if hit is not None and miss is not None and hit + miss > 0:
            notes.append(f"L2 hit rate = {hit / (hit + miss):.3f}")
        f.write("\n" + "; ".join(notes) + "\n\n")
print("wrote", f"{tag}_bwd_counters.md")

# what the operators sit inside: eager step of the NeRF fit / image fit, kernel time vs wall time
def step_md(w, title, fname, hot=("hashgrid_fwd", "untranspose_feats", "ctx_", "front16", "bin_", "zero_", "direct_accumulate", "transpose_grad")):
    jp = os.path.join(src, f"step_{w}.json")
    fs = glob.glob(os.path.join(src, f"step_{w}", "*/*kernel_stats.csv"))
    if not os.path.exists(jp) or not fs:
        return
    try:
        rec = json.loads([l for l in open(jp).read().splitlines() if l.startswith("{")][-1])
    except (IndexError, ValueError):
        return
    rows = list(csv.DictReader(open(max(fs, key=os.path.getmtime))))
    steps = rec.get("steps_traced", rec["steps"])
    tot = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / steps
    hot_us = sum(float(r["TotalDurationNs"]) for r in rows if any(h in r["Name"] for h in hot)) / 1e3 / steps
    prof_wall = rec["ms_per_step"] * 1e3
    wall, plain = prof_wall, False
    pp = os.path.join(src, f"step_{w}_plain.json")     # the same loop without the profiler attached
    if os.path.exists(pp):
        try:
            wall = json.loads([l for l in open(pp).read().splitlines() if l.startswith("{")][-1])["ms_per_step"] * 1e3
            plain = True
        except (IndexError, ValueError, KeyError):
            pass
    with open(os.path.join(out, fname), "w") as f:
        f.write(f"# {title}\n\n`rocprofv3 --kernel-trace --stats -- python3 tools/step_breakdown.py {w} {rec['steps']}` ({tag}, source hash "
                f"{kernel_source_hash()}).\n\n")
        f.write(f"Wall time per step (the loop's own clock, " + (f"a run WITHOUT the profiler; {prof_wall:.0f} us under it" if plain else "under the profiler, which inflates it") + f"): **{wall:.0f} us**. GPU kernel time per step (every "
                f"kernel of the trace, setup and validation included): **{tot:.0f} us**  -> the GPU is busy "
                f"{min(tot / wall, 1.0) * 100:.0f} % of the step; the rest is host time between launches (Python, autograd, "
                f"allocator, launch latency).\nHash-grid operators (forward + backward kernels of this library's hot path): "
                f"**{hot_us:.0f} us** per step = {hot_us / wall * 100:.0f} % of the wall time, {hot_us / max(tot, 1e-9) * 100:.0f} % of the kernel time.\n\n")
        f.write("| kernel | us per step | calls per step |\n|---|---|---|\n")
        for r in rows[:28]:
            f.write(f"| `{r['Name'][:100]}` | {float(r['TotalDurationNs']) / 1e3 / steps:.1f} | {int(r['Calls']) / steps:.1f} |\n")
    print("wrote", fname, "wall", wall, "kernels", tot, "hot", hot_us)

step_md("nerf", "NeRF-style render-and-fit (harness.fit_nerf), one eager training step", f"{tag}_nerf_step.md")
step_md("image", "Config-B image fit (harness.fit_image, 512x768), one eager training step", f"{tag}_imagefit_step.md")
step_md("image_graphed", "Config-B image fit, the step replayed from a HIP graph (GraphedImageFitter)", f"{tag}_imagefit_graphed_step.md")
step_md("nerf_pool", "NeRF-style render-and-fit fed from a resident ray pool (harness.fit_nerf(ray_pool=128)), one eager training step", f"{tag}_nerf_pool_step.md")
step_md("nerf_graphed", "NeRF-style render-and-fit, the step replayed from HIP graphs (GraphedNerfFitter, ray pool of 128 batches)", f"{tag}_nerf_graphed_step.md")

# MFMA utilisation of the decoder kernels (width 64 and 128)
mf = ctr("ctr_mlp128")
if mf:
    with open(os.path.join(out, f"{tag}_mlp_mfma_util.md"), "w") as f:
        f.write(f"# Decoder MLP kernels, matrix-core utilisation ({tag})\n\n`rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES "
                "SQ_WAVE_CYCLES SQ_INSTS_VALU GRBM_GUI_ACTIVE --kernel-trace -- python3 tools/mlp128_check.py` (averages over all "
                "launches of a kernel; batch sizes 65 536 / 409 600 / 2^20 mixed). MFMA busy = SQ_VALU_MFMA_BUSY_CYCLES / "
                "(GRBM_GUI_ACTIVE / 8 XCDs x 256 CUs x 4 SIMDs) is not exact for mixed launches; the ratio to SQ_BUSY_CYCLES is "
                "given as well.\n\n| kernel | MFMA busy cycles | SQ busy cycles | GRBM_GUI_ACTIVE | MFMA busy / (GUI/8 x 1024 SIMDs) |\n|---|---|---|---|---|\n")
        for k, d in mf.items():
            if "mlp" not in k:
                continue
            gui = d.get("GRBM_GUI_ACTIVE", 0.0)
            util = d.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (gui / 8 * 1024) if gui else float("nan")
            f.write(f"| `{k[:90]}` | {d.get('SQ_VALU_MFMA_BUSY_CYCLES', 0):,.0f} | {d.get('SQ_BUSY_CYCLES', 0):,.0f} | {gui:,.0f} | {util:.2f} |\n")
        f.write("\nAccuracy columns of the run below (round 4): against the SAME layers in float64, after dropping the rows whose ReLU "
                "branch differs from the fp64 evaluation (a pre-activation within rounding of 0 takes the other branch: an O(1) "
                "difference in that row's input gradient). The round-3 version of this table compared with torch's fp32 layers and "
                "did not drop those rows: its \"max rel grad diff\" of 1e-2..9e-2 were exactly such rows (1-12 per million samples "
                "here), not an error of the kernels; `tests/test_mlp.py::test_wide_decoders_at_nerf_batch_sizes` holds 1e-5 on every "
                "other row and on every weight gradient at 409 600 and 2^20 samples.\n")
        p2 = os.path.join(src, "mlp128_check.txt")
        if os.path.exists(p2):
            f.write("\n```\n" + open(p2).read() + "```\n")
    print("wrote", f"{tag}_mlp_mfma_util.md")
