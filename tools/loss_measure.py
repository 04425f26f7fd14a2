"""K1 (k_linearize) per loss at config 3, fp32: back-to-back h.linearize() launches timed with HIP events on the
handle's stream, as tools/k1_time.py does, one fresh process per leg, the legs alternated over three rounds.

  python tools/loss_measure.py [--parent-lib PATH] [--n 200] [--rounds 3]

Legs: huber on a parent library (--parent-lib, a libptzba.so built from the parent commit; its round-to-round spread
is the yardstick for "the existing instantiations did not change"), then huber, soft_l1, cauchy and arctan on this
tree's library.  Records profiles/loss_measure.json: per leg the us per launch of every round and repetition, the
medians of the rounds' medians, the ratios to huber and the parent's spread.  `--leg LOSS` is the child: one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ("huber", "soft_l1", "cauchy", "arctan")


def leg(loss, n, f_scale):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "pan-tilt-zoom-slam_amd"))
    import ptzba
    import synthetic
    p = synthetic.make_problem("config3", seed=0)
    h = ptzba.BAHandle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    ids = dict(linear=0, huber=1, soft_l1=2, cauchy=3, arctan=4)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=ptzba.FP32, loss=ids[loss],
                  f_scale=f_scale)
    h.set_state(p.init_ptz, p.init_rays)
    for _ in range(10):
        h.linearize()
    torch.cuda.synchronize()
    res = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            h.linearize()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / n)
    cost = float(h.read_scalars()[0])
    h.close()
    print(json.dumps(dict(loss=loss, us=res, cost=cost, problem=[p.n_pose, p.n_landmark, len(p.frame)])), flush=True)


def median(x):
    x = sorted(x)
    return x[len(x) // 2] if len(x) % 2 else 0.5 * (x[len(x) // 2 - 1] + x[len(x) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--parent-lib")
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f-scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_measure.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.n, a.f_scale)
    legs = ([("parent_huber", "huber", a.parent_lib)] if a.parent_lib else []) + [(k, k, None) for k in LOSSES]
    runs = {name: [] for name, _, _ in legs}
    for rnd in range(a.rounds):
        for name, loss, lib in legs:
            env = dict(os.environ)
            if lib:
                env["PTZBA_LIB"] = os.path.abspath(lib)
            else:
                env.pop("PTZBA_LIB", None)
            # a fresh process per leg; a leg that fails or hangs ends the measurement (nothing more is started)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", loss, "--n", str(a.n),
                                  "--f-scale", str(a.f_scale)], env=env, capture_output=True, text=True, timeout=120)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"leg {name} failed with {out.returncode}")
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            runs[name].append(rec)
            print(f"round {rnd} {name:13s} us per launch: " + " ".join(f"{x:.2f}" for x in rec["us"]), flush=True)
    # a leg's figure: the median of its rounds' medians (a round's first repetition is the slowest of its three)
    per_round = {name: [median(r["us"]) for r in rs] for name, rs in runs.items()}
    med = {name: median(v) for name, v in per_round.items()}
    result = dict(config="config3", precision="fp32", f_scale=a.f_scale, n=a.n, rounds=a.rounds, median_us=med,
                  per_round_median_us=per_round, ratio_to_huber={k: med[k] / med["huber"] for k in LOSSES},
                  runs=runs)
    if a.parent_lib:
        pr = per_round["parent_huber"]
        result["parent_spread_us"] = [min(pr), max(pr)]
        result["huber_inside_parent_spread"] = bool(min(pr) <= med["huber"] <= max(pr))
        result["huber_vs_parent"] = med["huber"] / med["parent_huber"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))


if __name__ == "__main__":
    main()
