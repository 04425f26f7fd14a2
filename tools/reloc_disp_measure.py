#!/usr/bin/env python3
"""What the displaced camera costs a pose-RANSAC call (ptz_pose_ransac / ptz_pose_ransac_disp), by
tools/pose_ransac_time.py's protocol: the call is synchronous (one upload, three launches, one download), so the time
is the wall clock around it; after 5 warm-ups, the median of 50 calls.  Legs, each a fresh process so that a leg loads
one library only:

  parent     the parent commit's library (--parent-lib), ptz_pose_ransac
  this       this tree's library without a displacement -- the same kernel instantiations as `parent`: must lie
             inside parent's own round-to-round spread
  this_disp  this tree's library with the golden fixtures' displacement (the scene seen through the displaced camera,
             reloc_disp_ref.make_scene_disp): recorded, not gated

The legs alternate for --rounds rounds inside one command.  Two shapes: the typical call (1000 correspondences, 1024
samples) and the GPU test's case 1 (96 correspondences, 256 samples); half of the correspondences are wrong, noise
0.5 px, threshold 3 px.  Writes profiles/reloc_disp_measure.json.

    python tools/reloc_disp_measure.py --parent-lib /path/to/parent/libptzba.so [--out out.json] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"parent": dict(parent=True, disp=False), "this": dict(parent=False, disp=False),
        "this_disp": dict(parent=False, disp=True)}
SHAPES = (("typical", 31, 1000, 1024), ("test_case_1", 11, 96, 256))


def leg(name, calls, warmup):
    for p in (os.path.join(ROOT, "pan-tilt-zoom-slam_amd"), os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, p)
    import numpy as np
    import pose_ransac_ref as pr
    import ptzba
    import reloc_disp_ref as rd
    from disp_ref import LAMBDA
    u, v = 640.0, 360.0
    disp = LEGS[name]["disp"]
    out = dict(leg=name, library=ptzba.lib().ptzba_version().decode(), displacement=disp, calls=calls, shapes={})
    for shape, scene_seed, n, n_hyp in SHAPES:
        gt, rays, pts, truth = (rd.make_scene_disp if disp else pr.make_scene)(scene_seed, n, 0.5, 0.5)
        kw = dict(threshold=3.0, n_hyp=n_hyp, seed=7)
        if disp:
            kw["displacement"] = LAMBDA
        for _ in range(warmup):
            r = ptzba.pose_ransac(u, v, rays, pts, **kw)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            r = ptzba.pose_ransac(u, v, rays, pts, **kw)
            t.append(time.perf_counter() - t0)
        out["shapes"][shape] = dict(n_corr=n, n_hyp=n_hyp, call_us_median=1e6 * statistics.median(t),
                                    call_us_min=1e6 * min(t), call_us_max=1e6 * max(t), found=bool(r.found),
                                    n_inliers=r.n_inliers, hyp_inliers=r.hyp_inliers, true_inliers=int(truth.sum()),
                                    pose_error=None if r.ptz is None else [float(x) for x in np.abs(r.ptz - gt)])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_disp_measure.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.calls, a.warmup)
    order = [n for n in ("parent", "this", "this_disp") if n != "parent" or a.parent_lib]
    runs = []
    for rnd in range(a.rounds):
        for name in order:
            env = dict(os.environ)
            env.pop("PTZBA_LIB", None)
            if LEGS[name]["parent"]:
                env["PTZBA_LIB"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--calls", str(a.calls),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"leg {name} failed with status {r.returncode}: nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["round"] = rnd
            print(json.dumps(rec), flush=True)
            runs.append(rec)
    summary = {}
    for shape, _, _, _ in SHAPES:
        s = {}
        for name in order:
            v = [r["shapes"][shape]["call_us_median"] for r in runs if r["leg"] == name]
            s[name] = dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)
        if "parent" in s:
            s["parent_spread_us"] = s["parent"]["max"] - s["parent"]["min"]
            s["this_minus_parent_us"] = s["this"]["median"] - s["parent"]["median"]
            s["this_inside_parent_spread"] = s["parent"]["min"] <= s["this"]["median"] <= s["parent"]["max"]
        s["disp_minus_no_disp_us"] = s["this_disp"]["median"] - s["this"]["median"]
        summary[shape] = s
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/reloc_disp_measure.py", calls=a.calls, warmup=a.warmup, rounds=a.rounds,
                       summary=summary, runs=runs), f, indent=1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
