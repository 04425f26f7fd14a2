"""Host-level checks of Map(ba_displacement=...): the camera's displacement reaches bundle_adjustment's displacement=
on every bundle adjustment of the map -- the first and the later ones, whose keyframes are the new objects the
previous call handed back -- with and without a window, and only when the option is on.  The solve is stubbed; no GPU."""
import numpy as np
import pytest

from disp_ref import LAMBDA


def _kf(i, displacement=None):
    from key_frame import KeyFrame
    k = KeyFrame(i, 100 + i, np.zeros(3), np.eye(3), 640.0, 360.0, 10.0 + 2.0 * i, -8.0, 3000.0)
    if displacement is not None:
        k.displacement = displacement
    return k


def _run(monkeypatch, n_calls=1, first=None, later=None, **map_kw):
    """A Map with the solve stubbed, one first keyframe (carrying `first` as its displacement) and n_calls
    add_keyframe_with_ba calls (their keyframes carrying `later`).  Returns (the keyword arguments of every
    bundle_adjustment call, the number of images of each, the map)."""
    import scene_map
    from key_frame import KeyFrame
    seen, sizes = [], []

    def stub(images, image_indices, feature_method, initial_ptzs, center, rotation, u, v, save_path, verbose=False,
             **kw):
        seen.append(kw)
        sizes.append(len(images))
        kfs = []
        for im, ix, ptz in zip(images, image_indices, initial_ptzs):  # new objects with features, as the real call's
            k = KeyFrame(im, ix, center, rotation, u, v, *ptz)
            k.set_features_lazy(np.zeros((2, 2)), np.zeros((2, 128), np.float32), np.arange(2))
            kfs.append(k)
        out = (np.zeros((0, 2)), kfs)
        if kw.get("marginalize") is not None:
            out += (dict(marginal=None, stats={}),)
        return out

    monkeypatch.setattr(scene_map, "bundle_adjustment", stub)
    m = scene_map.Map("sift", cache_correspondences=False, **map_kw)
    m.add_first_keyframe(_kf(0, first))
    for c in range(n_calls):
        m.add_keyframe_with_ba(_kf(1 + c, later), "")
    assert len(seen) == n_calls
    return seen, sizes, m


@pytest.mark.parametrize("window", [None, 3])
def test_every_bundle_adjustment_of_the_map_gets_the_displacement(monkeypatch, window):
    """Four successive calls, unwindowed and with a 3-keyframe window (the first keyframe, which carried the
    displacement, has left the window by the third call): displacement= on each, and on the keyframes kept."""
    seen, sizes, m = _run(monkeypatch, 4, first=LAMBDA.tolist(), ba_displacement=True, max_ba_frame=window)
    assert sizes == ([2, 3, 4, 5] if window is None else [2, 3, 3, 3])
    for kw in seen:
        np.testing.assert_array_equal(kw["displacement"], LAMBDA)
        assert kw["displacement"].dtype == np.float64
    assert len(m.keyframe_list) == 5
    for k in m.keyframe_list[-(window or 5):]:
        np.testing.assert_array_equal(k.displacement, LAMBDA)


def test_displacement_given_to_the_map_or_found_on_a_later_keyframe(monkeypatch):
    """Six values passed to Map reach every call whatever the keyframes carry; with True and a first keyframe without
    one, the first keyframe that carries a displacement supplies it from then on."""
    seen, _, _ = _run(monkeypatch, 3, ba_displacement=LAMBDA)
    assert all(np.array_equal(kw["displacement"], LAMBDA) for kw in seen)
    seen, _, _ = _run(monkeypatch, 3, first=None, later=LAMBDA, ba_displacement=True)
    assert all(np.array_equal(kw["displacement"], LAMBDA) for kw in seen)
    import scene_map
    for bad in (np.zeros(6), [1.0, 2.0], [0, 0, np.nan, 0, 0, 0]):
        with pytest.raises(ValueError, match="ba_displacement"):
            scene_map.Map("sift", ba_displacement=bad)


@pytest.mark.parametrize("map_kw,first", [({}, LAMBDA), (dict(ba_displacement=False), LAMBDA),
                                          (dict(ba_displacement=True), None), (dict(ba_displacement=True), np.zeros(6))])
def test_map_default_and_empty_displacement_pass_nothing(monkeypatch, map_kw, first):
    """Off by default; with the option on, keyframes without a displacement or with an all-zero one pass none (the
    rule of PtzSlam._disp), on the first call and on the later ones."""
    seen, _, _ = _run(monkeypatch, 3, first=first, **map_kw)
    assert all("displacement" not in kw for kw in seen)
