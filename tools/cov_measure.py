"""Time ptzba_covariance on the GPU (HIP events on the handle's stream, reported by the call itself): warm-up, repeated
runs, median.  Shapes: config 3 fp32 + Huber (poses only; poses + every ray) and config 2 fp64.  Next to each: the
same handle's LM time per trial, and the fp64 matrix-core rate of k_cov_gram -- its time taken as the call with the
blocks minus the call with none (same stream, the rest of the call identical), its work counted as 2 * 32^3 per visited
tile product (L_ik Z_k, M_i B_i and Z_i^T Z_i) from the factor's tile pattern.  Writes profiles/cov_measure.json.

    python tools/cov_measure.py [out.json] [repeats]

`joint` times ptzba_covariance_joint the same way at config 3 (fp32 + Huber) for three selections -- one frame + 500
rays (1,003 columns), every free pose (1,497 columns), two frames -- next to ptzba_covariance's figures of the same
run, and writes profiles/cov_joint_measure.json; `joint-fold` adds the two stages' kernel times from a
rocprofv3 --kernel-trace CSV of a separate run (main_joint).
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pan-tilt-zoom-slam_amd"))
import ptzba  # noqa: E402
import synthetic  # noqa: E402

NB = 32
FP64_MATRIX_PEAK_TFLOPS = 78.6  # MI355X fp64 matrix peak (the figure DESIGN.md 4.3 rates the factorisation against)
POSE_F, RAY_L = 10, 16          # frames / landmarks per right-hand-side block (csrc/ptzba_kernels.h, cov_kernels.hip)


def tile_pattern(pos, win, n_fixed, n_aug):
    """Strictly lower tiles of the factor's pattern with fill (chol_plan.cpp make_plan), rows < ceil(n_aug / 32)."""
    T = (n_aug + 1 + NB - 1) // NB
    nz = np.zeros((T, T), bool)
    n = len(pos)
    for f1 in range(n_fixed, n):
        for f2 in range(f1, min(n - 1, int(win[f1])) + 1):
            for a in (pos[f2], pos[f2] + 2):
                for b in (pos[f1], pos[f1] + 2):
                    i, j = max(a, b) // NB, min(a, b) // NB
                    nz[i, j] = True
    nz[n_aug // NB, :n_aug // NB + 1] = True
    for k in range(T):
        r = np.flatnonzero(nz[k + 1:, k]) + k + 1
        for x in r:
            nz[x, r[r <= x]] = True
    Tw = (n_aug + NB - 1) // NB
    return [np.flatnonzero(nz[i, :i]) for i in range(Tw)]


def products(rows, t0s):
    """Tile products of the blocks whose first tiles are t0s: per row tile i >= t0 its pattern tiles k in [t0, i),
    the diagonal-inverse product and the Gram product."""
    T = len(rows)
    per_t0 = [sum(int(np.count_nonzero(rows[i] >= t0)) + 2 for i in range(t0, T)) for t0 in range(T + 1)]
    return int(sum(per_t0[t] for t in t0s))


def block_first_tiles(p, pos, landmarks):
    free = np.sort(pos[pos >= 0])
    pose_t0 = [int(free[k]) // NB for k in range(0, len(free), POSE_F)]
    lm_min = np.full(p.n_landmark, np.iinfo(np.int64).max, np.int64)
    m = pos[p.frame] >= 0
    np.minimum.at(lm_min, p.landmark[m], pos[p.frame[m]].astype(np.int64))
    ray_t0 = []
    for b in range(0, len(landmarks), RAY_L):
        lo = lm_min[landmarks[b:b + RAY_L]].min()
        ray_t0.append(int(lo) // NB if lo < np.iinfo(np.int64).max else 1 << 30)
    return pose_t0, ray_t0


def measure(cfg, precision, loss, repeats):
    p = synthetic.make_problem(cfg, seed=0)
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision, loss=loss, f_scale=1.0)
    h.set_state(p.init_ptz, p.init_rays)
    h.save_state()
    si = h.solver_info()
    win = ptzba.frame_coupling_window(p.n_pose, p.frame, p.landmark)
    pos = ptzba.plan_export(win)[0]
    rows = tile_pattern(pos, win, 1, si["n_aug"])
    pose_t0, ray_t0 = block_first_tiles(p, pos, np.arange(p.n_landmark))
    T = len(rows)
    ray_t0 = [t for t in ray_t0 if t < T]

    def timed(**kw):
        for _ in range(3):
            h.covariance(**kw)
        return statistics.median(h.covariance(**kw)[2]["device_ms"] for _ in range(repeats))

    base = timed(landmarks=None, poses=False)
    poses = timed(landmarks=None)
    full = timed(landmarks="all")
    h.solve_resident(restore=True, max_iter=5)
    lm = [h.solve_resident(restore=True, max_iter=5) for _ in range(repeats)]
    lm_ms = statistics.median(1e3 * r.time / max(r.trials, 1) for r in lm)
    h.close()
    n_pose_prod, n_all_prod = products(rows, pose_t0), products(rows, pose_t0 + ray_t0)

    def rate(n_prod, ms):
        return 2.0 * NB ** 3 * n_prod / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")

    out = dict(config=cfg, precision="fp32" if precision == ptzba.FP32 else "fp64",
               loss="huber" if loss == ptzba.LOSS_HUBER else "linear", n_pose=p.n_pose, n_landmark=p.n_landmark,
               n_aug=si["n_aug"], ld=si["ld"], ordering=si["ordering"], row_tiles=T,
               pattern_tiles_lower=int(sum(len(r) for r in rows)), repeats=repeats,
               cov_ms_no_blocks=base, cov_ms_poses=poses, cov_ms_poses_all_rays=full,
               lm_ms_per_trial_host_wall=lm_ms,
               gram_ms_poses=poses - base, gram_ms_poses_all_rays=full - base,
               pose_blocks=len(pose_t0), ray_blocks=len(ray_t0),
               tile_products_poses=n_pose_prod, tile_products_poses_all_rays=n_all_prod,
               gram_tflops_poses=rate(n_pose_prod, poses - base),
               gram_tflops_poses_all_rays=rate(n_all_prod, full - base),
               fp64_matrix_peak_tflops=FP64_MATRIX_PEAK_TFLOPS)
    out["gram_peak_fraction_poses_all_rays"] = out["gram_tflops_poses_all_rays"] / FP64_MATRIX_PEAK_TFLOPS
    return out


def joint_shapes(p):
    """The joint call's timed selections at a problem: one frame + 500 rays (the EKF layout at R = 500: the last frame
    and the landmarks it sees first, filled up with others), every free pose, two frames."""
    f = p.n_pose - 1
    seen = np.unique(p.landmark[p.frame == f])
    rest = np.setdiff1d(np.arange(p.n_landmark), seen)
    rays = np.concatenate([seen, rest])[:500]
    return [("one_frame_500_rays", [f], rays), ("all_free_poses", np.arange(1, p.n_pose), []),
            ("two_frames", [1, f], [])]


def measure_joint(repeats):
    """ptzba_covariance_joint at config 3 (fp32 + Huber): HIP events around the whole call (its device_ms), 3 warm-up
    calls, median of `repeats`; next to it ptzba_covariance's figures of the same run."""
    p = synthetic.make_problem("config3", seed=0)
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=ptzba.FP32,
                  loss=ptzba.LOSS_HUBER, f_scale=1.0)
    h.set_state(p.init_ptz, p.init_rays)
    si = h.solver_info()

    def timed(call, **kw):
        for _ in range(3):
            call(**kw)
        return statistics.median(call(**kw)[-1]["device_ms"] for _ in range(repeats))

    base = timed(h.covariance, landmarks=None, poses=False)
    out = dict(config="config3", precision="fp32", loss="huber", n_pose=p.n_pose, n_landmark=p.n_landmark,
               n_aug=si["n_aug"], row_tiles=(si["n_aug"] + NB - 1) // NB, repeats=repeats, cov_ms_no_blocks=base,
               cov_ms_poses=timed(h.covariance, landmarks=None), cov_ms_poses_all_rays=timed(h.covariance, landmarks="all"),
               joint=[])
    for name, frames, rays in joint_shapes(p):
        ms = timed(h.covariance_joint, frames=frames, landmarks=rays)
        n_free = int(np.count_nonzero(np.asarray(frames) >= 1))
        blocks = (n_free + POSE_F - 1) // POSE_F + (len(rays) + RAY_L - 1) // RAY_L
        out["joint"].append(dict(shape=name, columns=3 * len(frames) + 2 * len(rays), column_blocks=blocks,
                                 block_pairs=blocks * (blocks + 1) // 2,
                                 z_workspace_bytes=blocks * out["row_tiles"] * NB * NB * 8,
                                 joint_ms=ms, stages_ms=ms - base))
    h.close()
    return out


def fold_kernel_trace(res, csv_path):
    """Adds each shape's median kernel time of stage 1 (k_cov_gram keeping Z) and stage 2 (k_cov_cross) from a
    rocprofv3 --kernel-trace CSV of a separate run of this tool; a shape's dispatches are told by their grid (one
    workgroup of 256 per column block in x)."""
    import csv
    st1, st2 = {}, {}
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            gx = int(row.get("Grid_Size_X", row.get("Grid_Size", 0)))
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3
            if "k_cov_cross" in name:
                st2.setdefault(gx // 256, []).append(us)
            elif "k_cov_gram" in name and ("true" in name or "Lb1" in name):
                st1.setdefault(gx // 256, []).append(us)
    for s in res["joint"]:
        b = s["column_blocks"]
        if b in st1 and b in st2:
            s["stage1_kernel_us"] = statistics.median(st1[b])
            s["stage2_kernel_us"] = statistics.median(st2[b])
            s["stage1_share"] = s["stage1_kernel_us"] / (s["stage1_kernel_us"] + s["stage2_kernel_us"])
            s["kernel_trace_dispatches"] = len(st2[b])
    return res


def main_joint(argv):
    """python tools/cov_measure.py joint [out.json] [repeats]: times the joint call, writes profiles/cov_joint_measure.json
    python tools/cov_measure.py joint-fold out.json kernel_trace.csv: folds a kernel trace's stage times into it"""
    default = os.path.join(ROOT, "profiles", "cov_joint_measure.json")
    if argv[0] == "joint-fold":
        with open(argv[1]) as f:
            doc = json.load(f)
        doc["config3"] = fold_kernel_trace(doc["config3"], argv[2])
    else:
        path = argv[1] if len(argv) > 1 else default
        repeats = int(argv[2]) if len(argv) > 2 else 15
        argv = [argv[0], path]
        doc = dict(tool="tools/cov_measure.py joint", version=ptzba.lib().ptzba_version().decode(),
                   config3=measure_joint(repeats))
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(argv[1])), exist_ok=True)
    with open(argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("joint", "joint-fold"):
        return main_joint(sys.argv[1:])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cov_measure.json")
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    res = []
    for cfg, prec, loss in (("config2", ptzba.FP64, ptzba.LOSS_LINEAR), ("config3", ptzba.FP32, ptzba.LOSS_HUBER)):
        r = measure(cfg, prec, loss, repeats)
        print(json.dumps(r), flush=True)
        res.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(tool="tools/cov_measure.py", version=ptzba.lib().ptzba_version().decode(), shapes=res), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
