"""Is K1 still the parent's K1, bit for bit and in time, after its two kernels' common pieces moved into
csrc/k1_device.h and the unlaunched global-table form of k_linearize went?  Two parts, each leg a fresh process that
loads one library only (PTZBA_LIB = --parent-lib for the parent's legs):

parity   The crafted problem of tests/k1_cases.py (~5,500 records, both table paths, four segment windows), unweighted and
         weighted, and a pair form of it (the first record of every segment, twice: every segment one run, so K1 is
         k_linearize_one, on both table paths as well), under three stream settings: the default (merged where the
         halving rule allows), PTZBA_K1_ONE=0 (the merged stream through the general kernel) and PTZBA_K1_MERGE=0 (the
         unmerged stream).  Per problem, precision
         (fp32, fp64), loss (the five) and displacement (cleared, set): linearise, build the reduced system at lambda 0
         and 1e-3 (the packed region of BAHandle.exchange() and read_scalars() after each build and solve), then one trial
         of the device-driven LM from the same state (read_scalars() and the state).  Every array is hashed; the parent's
         and this tree's hashes must be equal, leg by leg.

speed    config 3, fp32 + Huber, three streams: the pair form (k_linearize_one), the same input with PTZBA_K1_MERGE=0
         (k_linearize, unweighted) and the dedup form (k_linearize, weighted).  The libraries alternate for --rounds
         rounds; a leg reports K1's microseconds per launch inside device-resident solves (kernel_times()["linearize"])
         and the milliseconds per LM trial (event pair around each solve).  Pass: this tree's median is no slower than the
         parent's slowest round, per stream and figure.

    python tools/k1_share_measure.py --parent-lib /path/to/parent/libptzba.so [--out profiles/k1_share_measure.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = {"default": {}, "one_off": {"PTZBA_K1_ONE": "0"}, "merge_off": {"PTZBA_K1_MERGE": "0"}}
SPEED_STREAMS = {"pair": {}, "pair_merge_off": {"PTZBA_K1_MERGE": "0"}, "dedup": {}}
DISPLACEMENT = (0.01, -0.02, 0.03, 1e-5, -2e-5, 3e-5)  # tests/golden/make_golden.py's camera
MAX_ITER = 8


def _paths():
    for d in ("pan-tilt-zoom-slam_amd", "tests", ""):
        sys.path.insert(0, os.path.join(ROOT, d))


def _digest(*arrays):
    import numpy as np
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()[:16]


class DevArray:
    """__cuda_array_interface__ view of n doubles at a device pointer the library owns."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 3,
                                         "strides": None}


def pair_form(problem):
    """The first record of every (landmark, frame) segment of a k1_cases problem, twice, unweighted."""
    import numpy as np
    u, v, ptz0, rays0, frame, landmark, xy, _ = problem
    first = np.sort(np.unique(landmark.astype(np.int64) * len(ptz0) + frame, return_index=True)[1])
    twice = [np.repeat(a[first], 2, axis=0) for a in (frame, landmark, xy)]
    return (u, v, ptz0, rays0, *twice, None)


def parity_leg():
    """One library, one stream setting (the environment): every problem x precision x loss x displacement."""
    _paths()
    import numpy as np
    import torch
    import ptzba
    import k1_cases as kc
    problems = {"crafted": kc.craft(), "crafted_weighted": kc.craft(weighted=True), "pair": pair_form(kc.craft())}
    losses = {"linear": ptzba.LOSS_LINEAR, "huber": ptzba.LOSS_HUBER, "soft_l1": ptzba.LOSS_SOFT_L1,
              "cauchy": ptzba.LOSS_CAUCHY, "arctan": ptzba.LOSS_ARCTAN}
    out = {}
    for pname, (u, v, ptz0, rays0, frame, landmark, xy, weight) in problems.items():
        for prec_name, prec in (("fp32", ptzba.FP32), ("fp64", ptzba.FP64)):
            for lname, loss in losses.items():
                for disp in (False, True):
                    h = ptzba.BAHandle(0)
                    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=prec,
                                  loss=loss, f_scale=2.5)
                    if disp:
                        h.set_displacement(DISPLACEMENT)
                    h.set_state(ptz0, rays0)
                    h.save_state()
                    h.linearize()
                    sp, n, _ = h.exchange()
                    region = torch.as_tensor(DevArray(sp, n), device="cuda:0")
                    parts = [h.read_scalars()]
                    for lam in (0.0, 1e-3):
                        h.build_reduced(lam)
                        h.sync()
                        parts.append(region.cpu().numpy().copy())
                        h.solve_reduced()
                        parts.append(h.read_scalars())
                    res = h.solve_resident(restore=True, max_iter=1)
                    parts.append(h.read_scalars())
                    parts.extend(h.get_state())
                    mi = h.k1_merge_info()
                    key = f"{pname}/{prec_name}/{lname}/{'disp' if disp else 'nodisp'}"
                    out[key] = dict(sha=_digest(*parts), one_record=bool(mi["one_record"]), merged=bool(mi["merged"]),
                                    k1_groups_global=h.k1_info()[2], k1_windows=h.k1_info()[3], trials=res.trials,
                                    cost=float(parts[0][0]))
                    h.close()
    print(json.dumps(dict(library=ptzba.lib().ptzba_version().decode(), legs=out)), flush=True)


def speed_leg(stream, repeats):
    _paths()
    import torch
    import ptzba
    import synthetic
    p = synthetic.make_problem("config3", seed=0)
    frame, landmark, xy, w = p.frame, p.landmark, p.xy, None
    if stream == "dedup":
        frame, landmark, xy, w, _ = synthetic.dedup_records(frame, landmark, xy)
    h = ptzba.BAHandle(0)
    st = torch.cuda.Stream()
    h.set_stream(st.cuda_stream)
    h.set_problem(p.n_pose, p.n_landmark, frame, landmark, xy, p.u, p.v, weight=w, precision=ptzba.FP32,
                  loss=ptzba.LOSS_HUBER, f_scale=1.0)
    h.set_state(p.init_ptz, p.init_rays)
    h.save_state()
    for _ in range(3):
        h.solve_resident(restore=True, max_iter=MAX_ITER)
    ev_ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        res = h.solve_resident(restore=True, max_iter=MAX_ITER)
        e1.record(st)
        e1.synchronize()
        ev_ms.append(e0.elapsed_time(e1) / max(res.trials, 1))
    h.reset_kernel_times(True, groups=1)  # K1's own time: a pass of its own (the timer's events add gaps)
    for _ in range(3):
        h.solve_resident(restore=True, max_iter=MAX_ITER)
    k1_ms, k1_count = h.kernel_times()["linearize"]
    mi = h.k1_merge_info()
    h.reset_kernel_times(0)
    h.close()
    print(json.dumps(dict(stream=stream, library=ptzba.lib().ptzba_version().decode(), trials=res.trials,
                          ms_per_trial=statistics.median(ev_ms), k1_us_per_launch=1e3 * k1_ms, k1_launches=k1_count,
                          one_record=bool(mi["one_record"]), merged=bool(mi["merged"]))), flush=True)


def _child(args, env_extra, parent_lib):
    env = dict(os.environ)
    for k in ("PTZBA_LIB", "PTZBA_K1_ONE", "PTZBA_K1_MERGE"):
        env.pop(k, None)
    env.update(env_extra)
    if parent_lib:
        env["PTZBA_LIB"] = os.path.abspath(parent_lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"leg {args} failed with status {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["parity", "speed"])
    ap.add_argument("--stream")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k1_share_measure.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-speed", action="store_true")
    a = ap.parse_args()
    if a.leg == "parity":
        return parity_leg()
    if a.leg == "speed":
        return speed_leg(a.stream, a.repeats)
    if not a.parent_lib:
        raise SystemExit("--parent-lib is required: the comparison is against the parent's library")
    parity, differing = {}, []
    for sname, env in STREAMS.items():
        mine = _child(["--leg", "parity"], env, None)
        theirs = _child(["--leg", "parity"], env, a.parent_lib)
        for key, rec in mine["legs"].items():
            same = rec["sha"] == theirs["legs"][key]["sha"]
            parity[f"{sname}/{key}"] = dict(rec, parent_sha=theirs["legs"][key]["sha"], equal=same)
            if not same:
                differing.append(f"{sname}/{key}")
        print(f"parity {sname}: {len(mine['legs'])} legs, differing so far {len(differing)}", flush=True)
    speed, runs = {}, []
    if not a.skip_speed:
        for rnd in range(a.rounds):
            for sname, env in SPEED_STREAMS.items():
                # (the library that goes first alternates with the round: neither always runs on the warmer device)
                for who, lib in (("parent", a.parent_lib), ("this", None))[::-1 if rnd % 2 else 1]:
                    rec = _child(["--leg", "speed", "--stream", sname, "--repeats", str(a.repeats)], env, lib)
                    rec.update(who=who, round=rnd)
                    print(json.dumps(rec), flush=True)
                    runs.append(rec)
        for sname in SPEED_STREAMS:
            for fig in ("k1_us_per_launch", "ms_per_trial"):
                v = {who: [r[fig] for r in runs if r["stream"] == sname and r["who"] == who] for who in ("parent", "this")}
                speed[f"{sname}/{fig}"] = dict(parent_rounds=v["parent"], this_rounds=v["this"],
                                               parent_median=statistics.median(v["parent"]),
                                               parent_slowest=max(v["parent"]),
                                               this_median=statistics.median(v["this"]),
                                               within_parent_spread=statistics.median(v["this"]) <= max(v["parent"]))
    summary = dict(parity_legs=len(parity), parity_differing=differing,
                   speed_pass=all(s["within_parent_spread"] for s in speed.values()) if speed else None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/k1_share_measure.py", summary=summary, speed=speed, speed_runs=runs, parity=parity),
                  f, indent=1)
        f.write("\n")
    print(json.dumps(dict(summary=summary, speed=speed)))
    if differing:
        raise SystemExit(f"{len(differing)} parity legs differ from the parent")


if __name__ == "__main__":
    main()
