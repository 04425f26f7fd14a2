"""K2's producer / consumer kernel (k_schur_mfp, csrc/schur_kernels.hip: four staging waves, four product waves, an LDS
ring handed over through LDS counters) against the block-synchronous k_schur_mf it replaces (PTZBA_K2_PIPE=0): the same
arithmetic in the same order, so everything downstream is equal bit for bit -- the packed reduced system S | b | g_pose
| diag U at lambda 0 and 1e-3, an accepted device-driven LM trial (the alternate linearisation slot), and repeated
resident solves (no ring state survives a launch).  PTZBA_K2_PIPE=even (the other role placement) is held to the same.

BAHandle.k2_info() proves which pipeline shapes the problems run: one-batch items, odd and even batch counts, ragged
last batches, chunk-0 items (with the diagonal terms) and chunk > 0 items."""
import numpy as np
import pytest

import k1_cases as kc
from k2_cases import tiny as _tiny

pytestmark = pytest.mark.gpu

SETTINGS = ("0", None, "even")  # PTZBA_K2_PIPE: k_schur_mf, the default (waves 0-3 stage), the even waves stage
_cache = {}


def _problem(name):
    if name not in _cache:
        import synthetic
        if name == "tiny":
            _cache[name] = _tiny()
        elif name == "crafted":
            u, v, ptz0, rays0, frame, landmark, xy, _ = kc.craft()
            _cache[name] = dict(n_pose=len(ptz0), n_landmark=len(rays0), frame=frame, landmark=landmark, xy=xy, u=u, v=v,
                                ptz=ptz0, rays=rays0)
        else:
            p = (synthetic.make_grid_problem(120, 6000, -20.0, 20.0, (-10.0, 0.0, 10.0), seed=3) if name == "grid"
                 else synthetic.make_problem(name, seed=0))
            _cache[name] = dict(n_pose=p.n_pose, n_landmark=p.n_landmark, frame=p.frame, landmark=p.landmark, xy=p.xy,
                                u=p.u, v=p.v, ptz=p.init_ptz, rays=p.init_rays)
    return _cache[name]


def _open(p, loss, setting, monkeypatch):
    import ptzba
    if setting is None:
        monkeypatch.delenv("PTZBA_K2_PIPE", raising=False)
    else:
        monkeypatch.setenv("PTZBA_K2_PIPE", setting)
    h = ptzba.BAHandle(0)
    h.set_problem(p["n_pose"], p["n_landmark"], p["frame"], p["landmark"], p["xy"], p["u"], p["v"],
                  precision=ptzba.FP32, loss=ptzba.LOSS_HUBER if loss == "huber" else ptzba.LOSS_LINEAR)
    h.set_state(p["ptz"], p["rays"])
    return h


def _region(h):
    import torch
    import bench
    h.sync()
    sp, n, _ = h.exchange()
    return torch.as_tensor(bench._DevArray(sp, n), device="cuda:0").cpu().numpy().copy()


PROBLEMS = ("config2", "crafted", "grid", "tiny")


def test_problems_cover_the_pipeline_shapes(gpu_available, monkeypatch):
    """The four problems together run every shape of the hand-off: a single batch (nothing to re-fill), an odd batch
    count beyond it (the batch staged after the two-batch loop), an even one, ragged last batches, and items with
    and without the diagonal terms."""
    infos = {}
    for name in PROBLEMS:
        h = _open(_problem(name), "linear", None, monkeypatch)
        infos[name] = h.k2_info()
        h.close()
        print(f"K2PIPE k2_info {name}: {infos[name]}")
    for name, i in infos.items():
        assert i["items"] >= 1 and 1 <= i["nl_min"] <= i["nl_max"] <= 512, (name, i)
        assert i["nl_mod32_1_16"] + i["nl_mod32_17_31"] + i["nl_mod32_0"] == i["items"], (name, i)
        assert 1 <= i["chunk0_items"] <= i["items"], (name, i)
    t = infos["tiny"]
    assert t["nl_max"] <= 16 and t["nl_le16"] == t["items"] and t["chunk0_items"] < t["items"], t
    tot = {k: sum(i[k] for i in infos.values()) for k in infos["tiny"]}
    assert tot["nl_le16"] > 0                            # one batch
    assert tot["nl_mod32_1_16"] - tot["nl_le16"] > 0     # 3, 5, ... batches
    assert tot["nl_mod32_17_31"] + tot["nl_mod32_0"] > 0  # an even batch count
    assert tot["nl_mod32_17_31"] > 0                     # ... with a ragged last batch
    assert any(i["nl_min"] % 16 for i in infos.values())
    assert tot["chunk0_items"] > 0 and tot["items"] - tot["chunk0_items"] > 0
    assert infos["grid"]["nl_min"] > 4 * 16              # more batches than ring buffers: every item re-fills them


@pytest.mark.parametrize("loss", ["linear", "huber"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_reduced_system_bitwise_equal(gpu_available, name, loss, monkeypatch):
    p = _problem(name)
    out = []
    for setting in SETTINGS:
        h = _open(p, loss, setting, monkeypatch)
        h.linearize()
        regs = []
        for lam in (0.0, 1e-3):
            h.build_reduced(lam)
            regs.append(_region(h))
        out.append(regs)
        h.close()
    assert all(np.isfinite(r).all() for r in out[0]) and np.abs(out[0][0]).max() > 0
    for other, setting in zip(out[1:], SETTINGS[1:]):
        for ref, got, lam in zip(out[0], other, (0.0, 1e-3)):
            assert ref.shape == got.shape
            assert np.array_equal(ref, got), (name, loss, setting, lam, int(np.count_nonzero(ref != got)))


def test_alternate_slot_trial_bitwise_equal(gpu_available, monkeypatch):
    """One accepted device-driven LM trial: the build reads the linearisation slot the device chose (alt / sel)."""
    p = _problem("config2")
    out = []
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        r = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=1)
        out.append((h.get_state(), (r.cost, r.njev, r.nfev, r.status)))
        h.close()
    assert out[0][1][1] >= 1 and out[0][1][0] > 0
    for (ptz, rays), res in out[1:]:
        assert res == out[0][1]
        assert np.array_equal(ptz, out[0][0][0]) and np.array_equal(rays, out[0][0][1])
    assert not np.array_equal(out[0][0][0], p["ptz"])  # the trial was accepted: the state moved


def test_repeated_solves_bitwise_equal(gpu_available, monkeypatch):
    """Three restored solves of three LM iterations per handle: every launch starts from a clean ring."""
    p = _problem("config2")
    out = []
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        h.save_state()
        rs = [h.solve_resident(restore=True, ftol=1e-14, xtol=1e-16, max_iter=3) for _ in range(3)]
        out.append((h.get_state(), [(r.cost, r.njev, r.nfev, r.status) for r in rs]))
        h.close()
    assert out[0][1][0] == out[0][1][1] == out[0][1][2]
    for (ptz, rays), res in out[1:]:
        assert res == out[0][1]
        assert np.array_equal(ptz, out[0][0][0]) and np.array_equal(rays, out[0][0][1])
