"""
Map of keyframes and global ray landmarks (reference: slam_system/scene_map.py:18-168).

`Map.add_keyframe_with_ba` re-runs bundle adjustment over all keyframes, as the reference does
(scene_map.py:53-117), on the GPU.  `RandomForestMap` keeps the reference's sliding-window BA
(`bundle_adjustment_processing`, last `max_ba_frame` keyframes, scene_map.py:198-244).  The reference's
random-forest relocaliser (C++ rf_map via ctypes) is out of scope; `RandomForestMap.relocalize`
answers the same call with the nearest-neighbour ray map of nearest_neighbor.py and the two-point pose RANSAC
(ptzba.pose_ransac) in its place.

Both keep a correspondence.CorrespondenceCache keyed by KeyFrame.img_index: the reference re-detects
every keyframe and re-matches every pair on each BA call; here only the new keyframe is detected and
only its pairs are matched, with identical results.
"""
import time

import numpy as np
import scipy.io as sio

from bundle_adjustment import bundle_adjustment
from correspondence import CorrespondenceCache
from key_frame import KeyFrame
from util import overlap_pan_angle


class MarginalCarry:
    """The information a sliding window keeps of the keyframes that left it: one ptzba.Marginal keyed
    by image index.  Per BA call: `before(window image indices)` merges the marginal computed for a keyframe that has
    now left, conditions the stored factor on every keyframe outside the window at that keyframe's kept pose, and
    returns the factor to pass as bundle_adjustment's marginal_prior; `after(...)` records the poses of the call and
    the marginal of the window's first keyframe, which the next keyframe pushes out."""

    def __init__(self):
        self.stored = None
        self.pending = None  # (image index, Marginal): merged once that keyframe has left the window
        self.poses = {}      # image index -> (pan, tilt, f) as last adjusted

    def note(self, keyframes):
        for k in keyframes:
            self.poses[k.img_index] = (k.pan, k.tilt, k.f)

    def before(self, window):
        import ptzba
        window = set(window)
        if self.pending is not None:
            idx, m = self.pending
            if idx not in window and m is not None:
                self.stored = ptzba.merge_marginals(self.stored, m)
            self.pending = None
        if self.stored is not None:
            gone = [int(f) for f in self.stored.frames if int(f) not in window]
            if gone:
                self.stored = self.stored.condition(gone, np.array([self.poses[f] for f in gone], np.float64))
            if not len(self.stored.frames):
                self.stored = None
        return self.stored

    def after(self, keyframes, leaving, result):
        self.note(keyframes)
        if result is not None:
            self.pending = (leaving, result["marginal"])


class Map:
    """max_ba_frame: None (the reference: every keyframe is adjusted) or N: only the last N keyframes are
    adjusted, older ones stay as they are (RandomForestMap's window rule, scene_map.py:198-244; the
    streaming config's 30-keyframe window).  marginalize=True (with a window): the matches of the keyframe a full
    window is about to lose are turned into a prior on the keyframes that stay (MarginalCarry) instead of being thrown
    away.  ba_displacement: every bundle adjustment of the map runs under the camera's projection-centre displacement
    (the one the tracker projects with), bundle_adjustment's displacement=.  Six values, or True: the `displacement`
    attribute of the first keyframe that carries a non-zero one (read as PtzSlam._disp reads a camera's: all zero or
    missing is none).  The map keeps the value once it has it -- the keyframes a bundle adjustment hands back are new
    objects -- and copies it onto those keyframes.  reloc_displacement: relocalisation against this map
    (PtzSlam.relocalize -> relocalization_camera) runs under the displacement too.  Six values, or True: the value
    ba_displacement resolved to, or else the first keyframe's non-zero `displacement` attribute."""

    def __init__(self, feature_method, cache_correspondences=True, max_ba_frame=None, marginalize=False,
                 ba_displacement=False, reloc_displacement=False):
        assert feature_method in ("sift", "orb", "latch")
        self.global_ray = np.ndarray([0, 2])
        self.keyframe_list = []
        self.feature_method = feature_method
        self.ba_options = {}
        self.last_ba_time = None
        self.max_ba_frame = max_ba_frame
        self.correspondences = CorrespondenceCache() if cache_correspondences else None
        self.marginal_carry = MarginalCarry() if marginalize and max_ba_frame else None
        self.ba_displacement = None  # the six values, once known
        self._ba_displacement_from_keyframes = ba_displacement is True
        if ba_displacement is not True and ba_displacement is not False and ba_displacement is not None:
            self.ba_displacement = self._nonzero6(ba_displacement)
            if self.ba_displacement is None:
                raise ValueError("ba_displacement: six finite values, not all zero, expected (or True / False)")
        self.reloc_displacement = None  # the six values, once known
        self._reloc_displacement_from_map = reloc_displacement is True
        if reloc_displacement is not True and reloc_displacement is not False and reloc_displacement is not None:
            self.reloc_displacement = self._nonzero6(reloc_displacement)
            if self.reloc_displacement is None:
                raise ValueError("reloc_displacement: six finite values, not all zero, expected (or True / False)")

    @staticmethod
    def _nonzero6(d):
        """d as six float64 values, or None when it is missing, malformed or all zero."""
        if d is None:
            return None
        d = np.asarray(d, np.float64).reshape(-1)
        return d.copy() if d.shape == (6,) and np.isfinite(d).all() and np.any(d != 0) else None

    def _displacement_for_ba(self, keyframes):
        """The displacement of the next bundle adjustment (None: none); with ba_displacement=True it is looked for on
        the given keyframes until one carries it."""
        if self.ba_displacement is None and self._ba_displacement_from_keyframes:
            for k in keyframes:
                self.ba_displacement = self._nonzero6(getattr(k, "displacement", None))
                if self.ba_displacement is not None:
                    break
        return self.ba_displacement

    def displacement_for_reloc(self):
        """The displacement relocalisation runs under (None: none); with reloc_displacement=True the value the bundle
        adjustments use, or else that of the first keyframe that carries a non-zero one."""
        if self.reloc_displacement is None and self._reloc_displacement_from_map:
            self.reloc_displacement = self.ba_displacement
            for k in self.keyframe_list:
                if self.reloc_displacement is not None:
                    break
                self.reloc_displacement = self._nonzero6(getattr(k, "displacement", None))
        return self.reloc_displacement

    def add_first_keyframe(self, keyframe, verbose=False):
        assert isinstance(keyframe, KeyFrame)
        self.keyframe_list = [keyframe]
        if self.correspondences is not None and getattr(keyframe, "img", None) is not None:
            self.correspondences.prepare(keyframe.img_index, keyframe.img, self.feature_method)
        if verbose:
            print("first key frame is added, no bundle adjustment and landmark")

    def add_keyframe_without_ba(self, keyframe, verbose=False):
        assert isinstance(keyframe, KeyFrame)
        self.keyframe_list.append(keyframe)

    def add_keyframe_with_ba(self, keyframe, save_path, verbose=False, pose_prior=None):
        """scene_map.py:53-117: append, BA over all keyframes, keep keyframes with features.
        pose_prior: optional 3 x 3 covariance (pan, tilt, f) of the new keyframe's pose, e.g. the tracker's; the BA then
        carries the Gaussian prior with that covariance around the keyframe's current pose (bundle_adjustment's
        pose_priors)."""
        assert isinstance(keyframe, KeyFrame)
        assert len(self.keyframe_list) >= 1
        prior_kw = {}
        if pose_prior is not None:
            cov = np.asarray(pose_prior, np.float64)
            if cov.shape != (3, 3) or not np.isfinite(cov).all() or np.linalg.eigvalsh(0.5 * (cov + cov.T)).min() <= 0:
                raise ValueError("pose_prior must be a positive definite 3 x 3 covariance")
            info = np.linalg.inv(0.5 * (cov + cov.T))
            prior_kw = dict(pose_priors=[([keyframe.img_index], [keyframe.pan, keyframe.tilt, keyframe.f],
                                          0.5 * (info + info.T))])
        ref = self.keyframe_list[0]
        self.add_keyframe_without_ba(keyframe, False)
        kept = []
        if self.max_ba_frame and len(self.keyframe_list) > self.max_ba_frame:
            kept = self.keyframe_list[:-self.max_ba_frame]
            self.keyframe_list = self.keyframe_list[-self.max_ba_frame:]
            if self.correspondences is not None:
                self.correspondences.retain([k.img_index for k in self.keyframe_list])
        n = len(self.keyframe_list)
        images = [k.img for k in self.keyframe_list]
        image_indices = [k.img_index for k in self.keyframe_list]
        initial_ptzs = np.array([[k.pan, k.tilt, k.f] for k in self.keyframe_list], dtype=np.float64).reshape(n, 3)
        carry, leaving = self.marginal_carry, None
        if carry is not None:
            carry.note(kept + self.keyframe_list[:-1])
            prior_kw["marginal_prior"] = carry.before(image_indices)
            if n == self.max_ba_frame:
                leaving = image_indices[0]
                prior_kw["marginalize"] = [leaving]
        disp = self._displacement_for_ba([ref] + self.keyframe_list)
        if disp is not None:
            prior_kw["displacement"] = disp.copy()
        start = time.time()
        out = bundle_adjustment(images, image_indices, self.feature_method, initial_ptzs, ref.center,
                                ref.base_rotation, ref.u, ref.v, save_path, verbose,
                                correspondences=self.correspondences, **self.ba_options, **prior_kw)
        landmarks, keyframes = out[:2]
        end = time.time()
        if carry is not None:
            carry.after(keyframes, leaving, out[-1] if leaving is not None else None)
        self.keyframe_list.pop()
        self.global_ray = landmarks
        self.keyframe_list = list(kept)
        for i, kf in enumerate(keyframes):
            if disp is not None:
                kf.displacement = disp.copy()
            if kf.has_features():  # (get_feature_num() > 0 without forming the lists: they are formed on first use)
                self.keyframe_list.append(kf)
            else:
                print("warning: key frame, %d, image index %d is not included in the map" % (i, image_indices[i]))
        if verbose:
            print("updated map, number of key frame: %d, number of landmark %d" % (len(self.keyframe_list),
                                                                                 len(landmarks)))
        self.last_ba_time = end - start
        print("BA time", end - start)
        return landmarks, self.keyframe_list

    def good_new_keyframe(self, ptz, threshold1=5, threshold2=20, im_width=1280, verbose=False):
        """scene_map.py:119-149: max pan overlap with existing keyframes in (threshold1, threshold2)."""
        ptz = np.asarray(ptz)
        assert ptz.shape[0] == 3
        if len(self.keyframe_list) == 0:
            print("Warning: not existing key frames")
            return False
        ov = [overlap_pan_angle(ptz[2], ptz[0], k.f, k.pan, im_width) for k in self.keyframe_list]
        if verbose:
            print("candidate key frame overlap: ", ov)
        m = max(ov)
        return threshold1 < m < threshold2

    def save_keyframes_to_mat(self, path):
        kfs = [{"index": k.img_index, "ptz": np.array([k.pan, k.tilt, k.f]), "center": k.center,
                "base_rotation": k.base_rotation, "principal_point": np.array([k.u, k.v])} for k in self.keyframe_list]
        sio.savemat(path, mdict={"keyframes": kfs})


class RandomForestMap:
    """Sliding-window BA of scene_map.py:171-244: the last `max_ba_frame` keyframes are adjusted (the first
    of them is the gauge, bundle_adjustment fixes frame 0), older keyframes are kept as they are.  The
    random-forest map files (rf_map, C++) are not part of this build: `relocalize` searches a nearest-neighbour
    descriptor -> ray database over the keyframes (nearest_neighbor.NNBasedMap, exact kNN on the GPU) where the
    reference walks its forest, and estimates the pose from the matches by the two-point PTZ pose RANSAC where the
    reference runs its preemptive RANSAC (rf_map/util/ptz_pose_estimation.cpp).  reloc_displacement: `relocalize`
    builds its database and fits the pose under the camera's projection-centre displacement; six values, or True: the
    first keyframe's non-zero `displacement` attribute."""

    def __init__(self, max_ba_frame=10, feature_method="sift", cache_correspondences=True, reloc_displacement=False):
        self.keyframe_list = []
        self.feature_method = feature_method
        self.max_ba_frame = max_ba_frame
        self.global_ray = np.ndarray([0, 2])
        self.ba_options = {}
        self.correspondences = CorrespondenceCache() if cache_correspondences else None
        self.reloc_options = {}  # threshold / n_hyp / seed / ftol / xtol of relocalize's pose RANSAC
        self._nn_map = None  # the descriptor -> ray database of relocalize, rebuilt after add_keyframe
        self.reloc_displacement = None  # the six values, once known
        self._reloc_displacement_from_keyframes = reloc_displacement is True
        if reloc_displacement is not True and reloc_displacement is not False and reloc_displacement is not None:
            self.reloc_displacement = Map._nonzero6(reloc_displacement)
            if self.reloc_displacement is None:
                raise ValueError("reloc_displacement: six finite values, not all zero, expected (or True / False)")

    def displacement_for_reloc(self):
        """The displacement `relocalize` runs under (None: none)."""
        if self.reloc_displacement is None and self._reloc_displacement_from_keyframes:
            for k in self.keyframe_list:
                self.reloc_displacement = Map._nonzero6(getattr(k, "displacement", None))
                if self.reloc_displacement is not None:
                    break
        return self.reloc_displacement

    def add_keyframe(self, keyframe):
        self.keyframe_list.append(keyframe)
        self._drop_nn_map()
        if len(self.keyframe_list) > 1:
            self.bundle_adjustment_processing()

    def bundle_adjustment_processing(self, save_path="./bundle_result", verbose=False):
        ref = self.keyframe_list[0]
        n = len(self.keyframe_list)
        window = [k for i, k in enumerate(self.keyframe_list) if i >= n - self.max_ba_frame]
        kept = [k for i, k in enumerate(self.keyframe_list) if i < n - self.max_ba_frame]
        images = [k.img for k in window]
        idx = [k.img_index for k in window]
        ptzs = np.array([[k.pan, k.tilt, k.f] for k in window], dtype=np.float64)
        if self.correspondences is not None:
            self.correspondences.retain(idx)
        landmarks, kfs = bundle_adjustment(images, idx, self.feature_method, ptzs, ref.center, ref.base_rotation, ref.u,
                                           ref.v, save_path, verbose, correspondences=self.correspondences,
                                           **self.ba_options)
        self.global_ray = landmarks  # window-local ray ids (the reference discards them)
        self.keyframe_list = kept
        for i, kf in enumerate(kfs):
            if kf.get_feature_num() > 0:
                kf.convert_keypoint_to_array()
                self.keyframe_list.append(kf)
            else:
                print("warning: key frame, %d, image index %d is not included in the map" % (i, idx[i]))
        return landmarks, kfs

    def _drop_nn_map(self):
        if self._nn_map is not None:
            self._nn_map.close()
            self._nn_map = None

    def relocalize(self, keyframe, ptz):
        """The camera pose [3] of `keyframe` (its feature_pts / feature_des; its own pose is not read) against the
        keyframes of the map at their current, bundle-adjusted poses, or `ptz` when no pose is found."""
        if self._nn_map is None:
            from nearest_neighbor import NNBasedMap
            self._nn_map = NNBasedMap(displacement=self.displacement_for_reloc())
            self._nn_map.add_keyframes([k for k in self.keyframe_list if k.get_feature_num() > 0])
        pose, n_inliers, found = self._nn_map.relocalize_robust(keyframe, **self.reloc_options)
        return pose if found else np.asarray(ptz, np.float64)
