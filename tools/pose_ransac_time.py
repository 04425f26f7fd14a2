#!/usr/bin/env python3
"""Call time of ptzba.pose_ransac (ptz_pose_ransac) next to its NumPy restatement on the same inputs.

The entry point is synchronous (upload, three launches, one download), so the time is the wall clock around the
call: after a warm-up, the median of 50 calls.  Two shapes: the typical call (1000 correspondences, 1024 samples)
and the shape of the GPU test's case 1 (96 correspondences, 256 samples); half of the correspondences are wrong,
noise 0.5 px, threshold 3 px.  Prints one JSON line per shape.

    python tools/pose_ransac_time.py [--calls 50] [--warmup 5] [--no-numpy]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pan-tilt-zoom-slam_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy restatement")
    args = ap.parse_args()
    import numpy as np
    import pose_ransac_ref as pr
    import ptzba
    u, v = 640.0, 360.0
    for name, scene_seed, n, n_hyp in (("typical", 31, 1000, 1024), ("test_case_1", 11, 96, 256)):
        gt, rays, pts, truth = pr.make_scene(scene_seed, n, 0.5, 0.5)
        for _ in range(args.warmup):
            r = ptzba.pose_ransac(u, v, rays, pts, threshold=3.0, n_hyp=n_hyp, seed=7)
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            r = ptzba.pose_ransac(u, v, rays, pts, threshold=3.0, n_hyp=n_hyp, seed=7)
            t.append(time.perf_counter() - t0)
        out = {"shape": name, "n_corr": n, "n_hyp": n_hyp, "calls": args.calls,
               "gpu_call_us_median": round(1e6 * statistics.median(t), 1), "gpu_call_us_min": round(1e6 * min(t), 1),
               "gpu_call_us_max": round(1e6 * max(t), 1), "found": bool(r.found), "n_inliers": r.n_inliers,
               "hyp_inliers": r.hyp_inliers, "true_inliers": int(truth.sum()),
               "pose_error": None if r.ptz is None else [float(x) for x in np.abs(r.ptz - gt)]}
        if not args.no_numpy:
            t0 = time.perf_counter()
            ref = pr.pose_ransac_ref(u, v, rays, pts, 3.0, n_hyp, 7)
            out["numpy_restatement_s"] = round(time.perf_counter() - t0, 3)
            out["numpy_best_count"] = ref["cands"][ref["best"]][4]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
