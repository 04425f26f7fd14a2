"""What the keyframe marginalisation costs and what it changes (one GPU).  Writes profiles/marg_measure.json.

  time        ms per ptzba_marginal_prior call (HIP events on the handle's stream around the whole call, as the call
              reports them: 3 warm-up calls, the median of `repeats`), E = [0], at config 3 (fp32 + Huber) and at a
              30-keyframe window of the stream's shape (fp64, linear: 435 pairs capped at 200 matches, ~174K records),
              beside one LM trial on the same handle (cov_measure.py's method)
  regression  bench.py's ms_per_step for this tree's library and the parent commit's (--parent-lib), alternating inside
              this one command over --rounds rounds; no marginal and no priors set
  accuracy    demo_stream.py over --frames frames with and without --marginalize: pose RMSE against the truth and the
              keyframe-BA latency

Every leg that opens the GPU is a child process with its own time limit; after a leg that fails nothing more is started.

    python tools/marg_measure.py [--parent-lib /path/to/parent/libptzba.so] [--out out.json] [--repeats 15]
                                 [--rounds 3] [--frames 300] [--skip time,regression,accuracy]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pan-tilt-zoom-slam_amd")


def time_leg(repeats):
    sys.path.insert(0, PKG)
    import ptzba
    import synthetic
    shapes = []
    for name, make, prec, loss in (
            ("config3", lambda: synthetic.make_problem("config3", seed=0), ptzba.FP32, ptzba.LOSS_HUBER),
            ("window30", lambda: synthetic.make_small_problem(30, 4000, -20.0, 20.0, seed=0), ptzba.FP64, ptzba.LOSS_LINEAR)):
        p = make()
        h = ptzba.BAHandle(0)
        h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=prec, loss=loss, f_scale=1.0)
        h.set_state(p.init_ptz, p.init_rays)
        h.save_state()
        mask = ptzba.drop_mask(p.frame, [0])
        partners = np.unique(p.frame[mask != 0])
        partners = partners[partners != 0]
        if len(partners) > ptzba.MARG_MAX_FRAMES:  # (config 3: frame 0 overlaps more frames than a marginal may name)
            ok = np.isin(p.frame, np.concatenate([[0], partners[:ptzba.MARG_MAX_FRAMES]]))
            mask &= np.repeat(ok[0::2] & ok[1::2], 2).astype(np.uint8)
        for _ in range(3):
            m, st = h.marginal_prior([0], mask)
        ms = [h.marginal_prior([0], mask)[1]["device_ms"] for _ in range(repeats)]
        h.solve_resident(restore=True, max_iter=5)
        lm = [h.solve_resident(restore=True, max_iter=5) for _ in range(repeats)]
        h.close()
        shapes.append(dict(shape=name, precision="fp32" if prec == ptzba.FP32 else "fp64",
                           loss="huber" if loss == ptzba.LOSS_HUBER else "linear", n_pose=p.n_pose,
                           n_landmark=p.n_landmark, records=len(p.frame), dropped_records=st["dropped_records"],
                           dropped_landmarks=st["dropped_landmarks"], frames_in_marginal=len(m.frames), repeats=repeats,
                           marginal_prior_ms=statistics.median(ms), marginal_prior_ms_min=min(ms),
                           marginal_prior_ms_max=max(ms),
                           lm_ms_per_trial_host_wall=statistics.median(1e3 * r.time / max(r.trials, 1) for r in lm)))
    print(json.dumps(shapes), flush=True)


def child(cmd, env=None, limit=600):
    e = dict(os.environ)
    e.pop("PTZBA_LIB", None)
    e.update(env or {})
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)} failed with status {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marg_measure.json"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    if a.leg == "time":
        return time_leg(a.repeats)
    skip = set(a.skip.split(","))
    out = dict(tool="tools/marg_measure.py")
    py = sys.executable

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if "time" not in skip:
        out["time"] = child([py, os.path.abspath(__file__), "--leg", "time", "--repeats", str(a.repeats)])
        print(json.dumps(out["time"]), flush=True)
        save()
    if "regression" not in skip:
        runs = []
        for rnd in range(a.rounds):
            for name in (["parent"] if a.parent_lib else []) + ["this"]:
                env = {"PTZBA_LIB": os.path.abspath(a.parent_lib)} if name == "parent" else {}
                r = child([py, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "5"], env)
                runs.append(dict(leg=name, round=rnd, ms_per_step=r["ms_per_step"], value=r["value"]))
                print(json.dumps(runs[-1]), flush=True)
        reg = dict(runs=runs)
        for name in ("parent", "this"):
            v = [r["ms_per_step"] for r in runs if r["leg"] == name]
            if v:
                reg[name] = dict(median=statistics.median(v), min=min(v), max=max(v))
        if "parent" in reg:
            reg["this_minus_parent_ms"] = reg["this"]["median"] - reg["parent"]["median"]
            reg["parent_spread_ms"] = reg["parent"]["max"] - reg["parent"]["min"]
        out["regression"] = reg
        save()
    if "accuracy" not in skip:
        acc = {}
        for name, flag in (("plain", []), ("marginalize", ["--marginalize"])):
            r = child([py, os.path.join(PKG, "demo_stream.py"), "--frames", str(a.frames)] + flag, limit=900)
            acc[name] = dict(pose_rmse_vs_truth=r["pose_rmse_vs_truth"],
                             keyframe_pose_rmse_vs_truth=r.get("keyframe_pose_rmse_vs_truth"),
                             keyframe_ba_ms=r["keyframe_ba_ms"],
                             keyframes=r["keyframes"], lost_frames=r["lost_frames"], fps_end_to_end=r["fps_end_to_end"],
                             marginalize=r["marginalize"])
            print(json.dumps({name: acc[name]}), flush=True)
        out["accuracy"] = acc
        save()
    print(json.dumps({k: v for k, v in out.items() if k != "tool"}))


if __name__ == "__main__":
    main()
