"""What the ray priors cost per LM trial (config 3, fp32 + Huber, one GPU).  Legs, each a fresh process so that a leg
loads one library only:

  parent        the parent commit's library (--parent-lib), no priors
  this          this tree's library, no priors   -- queues no extra launch: must agree with `parent` within parent's
                                                    own round-to-round spread
  this_priors   this tree, a prior on every observed landmark (sigma 1e4 deg around the initial ray): one extra
                launch, k_ray_prior_apply, behind every linearisation; the fused prepare stays on.  The kernel's work
                does not depend on the values, and priors this weak leave the LM's trial sequence what it is without
                them, so the leg differs from `this` by the launch alone
  this_priors_stiff  the same with sigma 0.05 deg: priors that hold the rays at their (perturbed) initial values
                change the problem -- more trials per solve, a share of them rejected -- so its ms per trial spreads
                the solve's fixed start over another trial count: recorded, not compared

The legs alternate for --rounds rounds inside one command.  A leg warms up, then times `repeats` device-resident solves
(restore the saved state, a fixed number of LM iterations) with an event pair on the solve's stream around each, and
reports the median ms per LM trial (device timeline) beside the host wall time.  Writes
profiles/ray_prior_measure.json.

    python tools/ray_prior_measure.py --parent-lib /path/to/parent/libptzba.so [--out out.json] [--repeats 15] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {
    "parent": dict(parent=True, priors=False),
    "this": dict(parent=False, priors=False),
    "this_priors": dict(parent=False, priors=True, sigma=1e4),
    "this_priors_stiff": dict(parent=False, priors=True, sigma=0.05),
}
MAX_ITER = 8


def every_observed_ray(p, sigma):
    import numpy as np
    seen = np.flatnonzero(np.bincount(p.landmark, minlength=p.n_landmark) > 0)
    info = np.eye(2) / sigma ** 2
    return [(int(l), p.init_rays[l], info) for l in seen]


def leg(name, repeats):
    sys.path.insert(0, os.path.join(ROOT, "pan-tilt-zoom-slam_amd"))
    import torch
    import ptzba
    import synthetic
    p = synthetic.make_problem("config3", seed=0)
    h = ptzba.BAHandle(0)
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=ptzba.FP32,
                  loss=ptzba.LOSS_HUBER, f_scale=1.0)
    priors = every_observed_ray(p, LEGS[name]["sigma"]) if LEGS[name]["priors"] else []
    if priors:
        h.set_ray_priors(priors)
    h.set_state(p.init_ptz, p.init_rays)
    h.save_state()
    for _ in range(3):
        h.solve_resident(restore=True, max_iter=MAX_ITER)
    ev_ms, wall_ms, trials = [], [], []
    res = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        res = h.solve_resident(restore=True, max_iter=MAX_ITER)
        e1.record(stream)
        e1.synchronize()
        t = max(res.trials, 1)
        ev_ms.append(e0.elapsed_time(e1) / t)
        wall_ms.append(1e3 * res.time / t)
        trials.append(res.trials)
    out = dict(leg=name, library=ptzba.lib().ptzba_version().decode(), ray_priors=len(priors), repeats=repeats,
               trials_per_solve=trials[-1], iterations=res.iterations, cost=res.cost,
               ms_per_trial_events=statistics.median(ev_ms), ms_per_trial_events_min=min(ev_ms),
               ms_per_trial_events_max=max(ev_ms), ms_per_trial_wall=statistics.median(wall_ms),
               solver=h.solver_info())
    if priors:
        out["ray_prior_info"] = h.ray_prior_info()[:3]
    h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_prior_measure.json"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.repeats)
    order = [n for n in ("parent", "this", "this_priors", "this_priors_stiff") if n != "parent" or a.parent_lib]
    runs = []
    for rnd in range(a.rounds):
        for name in order:
            env = dict(os.environ)
            env.pop("PTZBA_LIB", None)
            if LEGS[name]["parent"]:
                env["PTZBA_LIB"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--repeats", str(a.repeats)],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"leg {name} failed with status {r.returncode}: nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["round"] = rnd
            print(json.dumps(rec), flush=True)
            runs.append(rec)

    def med(name):
        v = [r["ms_per_trial_events"] for r in runs if r["leg"] == name]
        return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v) if v else None

    summary = {n: med(n) for n in order}
    if summary.get("parent"):
        summary["this_minus_parent_ms"] = summary["this"]["median"] - summary["parent"]["median"]
        summary["parent_spread_ms"] = summary["parent"]["max"] - summary["parent"]["min"]
    summary["priors_minus_no_priors_ms"] = summary["this_priors"]["median"] - summary["this"]["median"]
    summary["trials_per_solve"] = {n: sorted({r["trials_per_solve"] for r in runs if r["leg"] == n}) for n in order}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/ray_prior_measure.py", config="config3", precision="fp32", loss="huber",
                       max_iter=MAX_ITER, summary=summary, runs=runs), f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
