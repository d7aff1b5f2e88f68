"""filter 'cubic' (IST_FILTER_CUBIC) on one MI355X: the streamed cubic path against bilinear on the same plan and against the
per-pixel general path.  Device-resident (sources and canvases in HBM, three buffer sets rotated, device events around back-to-back
launches, a pre-roll before every timed region).  Prints ONE JSON line.

Workloads (enlargements are what the reference's own small-job plan and mode 'max' produce: index.js:1363, 1426-1428):
  1  nine images of 1551x1163 to a 4032-wide vertical strip: a uniform 2.6x enlargement at the headline canvas size
  2  bench.py's mixed-size list under mode 'max', vertical (enlargements of 1.0-1.33x)
  3  plan golden G1 on the devtools plan: 3 x 640x480 under ctx.scale(2.6), edge AA on; tiny, so read it as latency

Arms, each in a child process of its own, rounds interleaved (the tuning knobs are read once per process):
  bilinear        the comparator: the same plan, the same bytes in and out
  cubic           the streamed path (PATH_CUBIC_STREAM)
  cubic_general   IST_TUNING=1 IST_NO_LDS=1: the same cells through the per-pixel paint stack
Reported per workload and arm: microseconds per stitch (median over rounds of the per-round medians) and the share of the HBM peak
over ist_job_info.algorithmic_bytes (the byte count bench.py uses); cubic / bilinear and cubic_general / cubic as ratios.

  python tools/bench_cubic.py [--rounds 2] [--workloads 123]
  rocprofv3 --kernel-trace --stats -d DIR -o cubic -- python tools/bench_cubic.py --child cubic --workloads 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = [("bilinear", "bilinear", {}), ("cubic", "cubic", {}), ("cubic_general", "cubic", {"IST_TUNING": "1", "IST_NO_LDS": "1"})]
WHAT = {"1": "9 x 1551x1163 -> 4032-wide vertical strip (2.6x)", "2": "bench.py MIXED, mode 'max', vertical (1.0-1.33x)",
        "3": "G1: 3 x 640x480, devtools plan (superSample 2.6, edge AA)"}


def workload(name):
    import bench
    if name == "1":
        return [(1551, 1163)] * 9, {"superSample": 2.6}                     # canvas floor(1551 * 2.6) = 4032 wide, k = 1 / 2.6 on both axes
    if name == "2":
        return list(bench.MIXED), {"mode": "max"}
    return [(640, 480)] * 3, {"platform": "devtools"}


def child(filt, workloads):
    """one arm: every workload under `filt`; prints {workload: {us, algorithmic_bytes, tiles_*}}"""
    import torch

    import bench
    import imagestitching_amd as ist
    assert torch.cuda.is_available(), "bench_cubic needs a GPU"
    dev = torch.device("cuda", 0)
    st = ist.Stitcher(0)
    out = {}
    for w in workloads:
        sizes, opts = workload(w)
        p, job = st.compile([{"width": a, "height": b, "opaque": True} for a, b in sizes], "vertical", dict(opts, filter=filt))
        nsets = 3
        sets = [[torch.randint(0, 256, (h, ww, 4), dtype=torch.uint8, device=dev) for (ww, h) in sizes] for _ in range(nsets)]
        outs = [torch.empty((p.canvas_h, p.canvas_w, 4), dtype=torch.uint8, device=dev) for _ in range(nsets)]
        state = {"i": 0}

        def step():
            i = state["i"] = (state["i"] + 1) % nsets
            job.launch(sets[i], outs[i])

        # one launch decides how many fit a timed window of about 0.2 s (the general path is orders slower than the streamed one)
        step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        steps = int(min(2000, max(5, 200.0 / max(e0.elapsed_time(e1), 1e-3))))
        bench.preroll(step, torch)
        samples = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / steps)
        out[w] = {"us": round(statistics.median(samples), 2), "us_samples": [round(v, 2) for v in samples], "steps": steps,
                  "algorithmic_bytes": int(job.info["algorithmic_bytes"]), "canvas": [p.canvas_w, p.canvas_h],
                  "tiles_sample": int(job.info["tiles_sample"]), "tiles_general": int(job.info["tiles_general"]), "tiles_copy": int(job.info["tiles_copy"])}
        job.close()
        del sets, outs
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--workloads", default="123")
    ap.add_argument("--child", default=None, help="run one arm in this process: the filter name")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.workloads)
        return
    import bench
    runs = {name: [] for name, _, _ in ARMS}
    for _ in range(args.rounds):
        for name, filt, env in ARMS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", filt, "--workloads", args.workloads],
                               env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
            if r.returncode != 0 or not r.stdout.strip():
                raise SystemExit("arm %s failed (exit %d): %s" % (name, r.returncode, r.stderr[-2000:]))
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = {"metric": "filter 'cubic': us per stitch, device-resident, against bilinear and the per-pixel general path",
            "rounds": args.rounds, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "kernel_source_sha": bench.kernel_source_sha()}
    for w in args.workloads:
        res = {"what": WHAT[w]}
        for name, _, _ in ARMS:
            per_round = [r[w]["us"] for r in runs[name]]
            us = statistics.median(per_round)
            first = runs[name][0][w]
            res[name] = {"us": round(us, 2), "us_per_round": per_round, "algorithmic_bytes": first["algorithmic_bytes"],
                         "hbm_frac": round(first["algorithmic_bytes"] / (us * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 4),
                         "tiles_sample": first["tiles_sample"], "tiles_general": first["tiles_general"], "tiles_copy": first["tiles_copy"]}
            res["canvas"] = first["canvas"]
        res["cubic_over_bilinear"] = round(res["cubic"]["us"] / res["bilinear"]["us"], 3)
        res["general_over_cubic"] = round(res["cubic_general"]["us"] / res["cubic"]["us"], 3)
        line["workload_" + w] = res
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
