"""What the projection-centre displacement costs per LM trial (config 3, fp32 + Huber, one GPU; DESIGN 4.8's
protocol).  Legs, each a fresh process so that a leg loads one library only:

  parent      the parent commit's library (--parent-lib), no displacement
  this        this tree's library, no displacement -- launches the same kernel instantiations as `parent`: must agree
              with it within parent's own round-to-round spread
  this_disp_tiny  this tree with ptzba_set_displacement(1e-9 x the golden fixtures' displacement): K1 runs its DISP
              instantiation (k_linearize_one at config 3) and nothing else changes.  The kernel's work does not depend
              on the values, and a displacement this small (1e-6 px) leaves the LM's trial sequence what it is without
              one, so the leg differs from `this` by the instantiation alone; recorded next to K1's own per-launch
              time (ptzba_kernel_times, a separate timed pass); not gated
  this_disp   the same with the golden fixtures' displacement itself.  The observations are config 3's own, rendered
              without a displacement, so this is another problem with another trial sequence (more trials per solve,
              a share of them rejected): recorded, not compared

The legs alternate for --rounds rounds inside one command.  A leg warms up, then times `repeats` device-resident solves
(restore the saved state, a fixed number of LM iterations) with an event pair on the solve's stream around each, and
reports the median ms per LM trial (device timeline) beside the host wall time; then three more solves with the K1
timer on give K1's mean microseconds per launch inside a solve, and 30 linearisations in a row at the initial state
give it at one fixed state.  Writes profiles/displacement_measure.json.

    python tools/displacement_measure.py --parent-lib /path/to/parent/libptzba.so [--out out.json] [--repeats 15] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {
    "parent": dict(parent=True, disp=False),
    "this": dict(parent=False, disp=False),
    "this_disp_tiny": dict(parent=False, disp=True, scale=1e-9),
    "this_disp": dict(parent=False, disp=True, scale=1.0),
}
DISPLACEMENT = (0.01, -0.02, 0.03, 1e-5, -2e-5, 3e-5)  # tests/golden/make_golden.py's camera
MAX_ITER = 8


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
    if LEGS[name]["disp"]:
        h.set_displacement([LEGS[name]["scale"] * d for d in DISPLACEMENT])
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
    # K1's own time per launch: a pass of its own with the kernel timer on (the event pairs add gaps to the stream)
    h.reset_kernel_times(True, groups=1)
    for _ in range(3):
        h.solve_resident(restore=True, max_iter=MAX_ITER)
    k1_ms, k1_count = h.kernel_times()["linearize"]  # (mean ms per timed launch, launches)
    # ... and K1 alone at one fixed state: the same launch 30 times in a row at the initial state, whatever trial
    # sequence the leg's solves take (tells the kernel's own cost from the launch mix of a solve)
    h.set_state(p.init_ptz, p.init_rays)
    h.linearize()
    h.reset_kernel_times(True, groups=1)
    for _ in range(30):
        h.linearize()
    k1_fixed_ms, k1_fixed_count = h.kernel_times()["linearize"]
    out = dict(leg=name, library=ptzba.lib().ptzba_version().decode(), displacement=bool(LEGS[name]["disp"]),
               repeats=repeats, trials_per_solve=trials[-1], iterations=res.iterations, cost=res.cost,
               ms_per_trial_events=statistics.median(ev_ms), ms_per_trial_events_min=min(ev_ms),
               ms_per_trial_events_max=max(ev_ms), ms_per_trial_wall=statistics.median(wall_ms),
               k1_us_per_launch=1e3 * k1_ms, k1_launches_timed=k1_count,
               k1_us_fixed_state=1e3 * k1_fixed_ms, k1_fixed_launches_timed=k1_fixed_count,
               k1_merge=h.k1_merge_info(), solver=h.solver_info())
    h.reset_kernel_times(0)
    h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "displacement_measure.json"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.repeats)
    order = [n for n in ("parent", "this", "this_disp_tiny", "this_disp") if n != "parent" or a.parent_lib]
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

    def med(name, key="ms_per_trial_events"):
        v = [r[key] for r in runs if r["leg"] == name]
        return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v) if v else None

    summary = {n: med(n) for n in order}
    summary["k1_us_per_launch"] = {n: med(n, "k1_us_per_launch") for n in order}
    summary["k1_us_fixed_state"] = {n: med(n, "k1_us_fixed_state") for n in order}
    if summary.get("parent"):
        summary["this_minus_parent_ms"] = summary["this"]["median"] - summary["parent"]["median"]
        summary["parent_spread_ms"] = summary["parent"]["max"] - summary["parent"]["min"]
    summary["disp_minus_no_disp_ms"] = summary["this_disp_tiny"]["median"] - summary["this"]["median"]
    summary["k1_disp_minus_no_disp_us"] = (summary["k1_us_per_launch"]["this_disp_tiny"]["median"] -
                                           summary["k1_us_per_launch"]["this"]["median"])
    summary["trials_per_solve"] = {n: sorted({r["trials_per_solve"] for r in runs if r["leg"] == n}) for n in order}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/displacement_measure.py", config="config3", precision="fp32", loss="huber",
                       max_iter=MAX_ITER, displacement=list(DISPLACEMENT), summary=summary, runs=runs), f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
