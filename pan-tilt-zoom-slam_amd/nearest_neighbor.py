"""
Nearest-neighbour relocalisation over the whole map (reference: slam_system/nearest_neighbor.py, NNBasedMap).

The map keeps one global descriptor -> ray database over all keyframes; a lost frame's descriptors are matched to it
by a 1-nearest-neighbour search and the camera's (pan, tilt, f) is fitted to the matched rays.  The reference
searches with FLANN's approximate kd-tree (pyflann, nearest_neighbor.py:30-35); here the search is the exact
brute-force kNN-2 kernel of the front-end (ptz_match_knn2_sets, first column) against a device-resident copy of
`global_des`, so `find_nearest` returns the true nearest row where FLANN may return a near one.  The acceptance rule
is the reference's: squared L2 distance < 2000 (FLANN's nn_index returns squared distances, nearest_neighbor.py:40).

`relocalize` is the reference's: a plain pose-only least squares from the keyframe's own pose over every match
(nearest_neighbor.py:86-122, without its .mat dump) -- it needs a close starting pose and has no defence against
wrong matches.  `relocalize_robust` needs neither: the matches go to the two-point PTZ pose RANSAC
(ptzba.pose_ransac), which samples pose candidates in closed form, scores them all and refits the best on its inliers.

`displacement=`: the camera's six projection-centre displacement values (the model the tracker and, with
ba_displacement, the bundle adjuster project with).  The map then stores the exact inverse projections of its
keyframes' features (ptzba.back_project_rays(exact=True); the reference's back_project_to_ray is only an approximate
inverse once the displacement is not zero), and both relocalisations fit the pose under the displaced model.
"""
import itertools

import numpy as np

import ptzba
from scene_map import Map


class NNBasedMap(Map):
    MAX_SQ_DIST = 2000.0  # nearest_neighbor.py:40
    _ids = itertools.count(1)  # device descriptor-set keys: a range of their own, two per instance

    def __init__(self, device=None, displacement=None):
        super().__init__('sift')
        self.displacement = None  # six values, or None (also for six zeros, as PtzSlam._disp reads a camera's)
        if displacement is not None:
            d = np.asarray(displacement, np.float64).reshape(-1)
            if d.shape != (6,) or not np.isfinite(d).all():
                raise ValueError("displacement: six finite values expected")
            self.displacement = d.copy() if np.any(d != 0) else None
        self.global_des = np.ndarray([0, 128], dtype=np.float32)  # [N, 128], row k belongs to global_ray[k]
        self.device = device
        k = next(NNBasedMap._ids)
        self._train_key = (1 << 62) + 2 * k
        self._query_key = self._train_key + 1
        self._resident_rows = None  # rows of global_des on the device (None: not uploaded)

    # ------------------------------------------------------------------ the database
    def build_kdtree(self):
        """Upload `global_des` as a device-resident descriptor set (what stands in for FLANN's build_index)."""
        self._resident_rows = ptzba.desc_put_new(self._train_key, np.asarray(self.global_des, np.float32).reshape(
            len(self.global_des), -1), self.device)

    def close(self):
        """Free the device descriptor sets of this map."""
        if self._resident_rows is not None:
            self._resident_rows = None
            ptzba.desc_drop([self._train_key, self._query_key], self.device)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def find_nearest(self, des):
        """1-NN of every query descriptor in `global_des`; a query is kept when the squared L2 distance is below
        2000.  Returns (matched_keypoint_index, matched_ray_index) in query order."""
        if self._resident_rows != len(self.global_des):
            self.build_kdtree()
        n = ptzba.desc_put_new(self._query_key, des, self.device)
        if n == 0 or self._resident_rows == 0:
            return [], []
        idx, dist = ptzba.match_knn2_sets([self._query_key], [n], self._train_key, self.device)
        d2 = dist[:, 0].astype(np.float64) ** 2
        keep = np.flatnonzero((idx[:, 0] >= 0) & (d2 < self.MAX_SQ_DIST))
        return keep.tolist(), idx[keep, 0].tolist()

    def add_keyframe_without_ba(self, keyframe, verbose=False):
        """nearest_neighbor.py:46-56: append the keyframe, its features' rays at its pose, and their descriptors.
        With a displacement the rays are the exact inverse projections, and a feature without a ray in the
        (theta, phi) chart is left out of global_ray and global_des together."""
        super().add_keyframe_without_ba(keyframe, verbose)
        pts = _points_array(keyframe.feature_pts)
        des = np.asarray(keyframe.feature_des, np.float32).reshape(len(pts), -1)
        if self.displacement is None:
            rays = ptzba.back_project_rays(keyframe.u, keyframe.v, keyframe.f, keyframe.pan, keyframe.tilt, pts)
        else:
            rays, valid = ptzba.back_project_rays(keyframe.u, keyframe.v, keyframe.f, keyframe.pan, keyframe.tilt, pts,
                                                  self.displacement, exact=True)
            rays, des = rays[valid], des[valid]
        self.global_ray = np.vstack([self.global_ray, rays])
        self.global_des = np.vstack([self.global_des, des])

    def add_keyframes(self, keyframe_list):
        for keyframe in keyframe_list:
            self.add_keyframe_without_ba(keyframe)
        self.build_kdtree()

    @staticmethod
    def compute_residual(pose, rays, points, u, v, displacement=None):
        """nearest_neighbor.py:64-83: interleaved reprojection errors of `rays` at `pose` against `points`; with
        displacement= (a map's `displacement`) under the displaced camera."""
        rays = np.asarray(rays, np.float64).reshape(-1, 2)
        points = np.asarray(points, np.float64).reshape(-1, 2)
        n = len(rays)
        if displacement is not None:
            xy = ptzba.project_rays(u, v, pose[2], pose[0], pose[1], rays, displacement)
            return (xy - points).reshape(-1)
        x, y = ptzba.ray_to_image(u, v, np.full(n, pose[2]), np.full(n, pose[0]), np.full(n, pose[1]), rays[:, 0],
                                  rays[:, 1])
        return np.stack([x - points[:, 0], y - points[:, 1]], 1).reshape(-1)

    # ------------------------------------------------------------------ relocalisation
    def _matches(self, keyframe):
        keypoint_index, ray_index = self.find_nearest(keyframe.feature_des)
        pts = _points_array(keyframe.feature_pts)
        return self.global_ray[ray_index].reshape(-1, 2), pts[keypoint_index].reshape(-1, 2)

    def relocalize(self, keyframe):
        """nearest_neighbor.py:86-122: least squares over every match, from the keyframe's own pose."""
        rays, points = self._matches(keyframe)
        pose = np.array([keyframe.pan, keyframe.tilt, keyframe.f], np.float64)
        if len(rays) == 0:
            return pose
        ptz, cost, its, status = ptzba.refine_poses(keyframe.u, keyframe.v, pose[None], rays, points, ftol=1e-4,
                                                    displacement=self.displacement)
        return ptz[0]

    def relocalize_robust(self, keyframe, threshold=3.0, n_hyp=1024, seed=0, ftol=1e-4, xtol=1e-8):
        """Pose of `keyframe` from its features alone (its pan / tilt / f are not read): find_nearest, then the
        two-point pose RANSAC (ftol, xtol: its refit's).  Returns (ptz [3] or None, inlier count, found)."""
        rays, points = self._matches(keyframe)
        if len(rays) < 2:
            return None, 0, False
        r = ptzba.pose_ransac(keyframe.u, keyframe.v, rays, points, threshold=threshold, n_hyp=n_hyp, seed=seed,
                              ftol=ftol, xtol=xtol, device=self.device, displacement=self.displacement)
        return r.ptz, r.n_inliers, r.found


def _points_array(feature_pts):
    if isinstance(feature_pts, np.ndarray):
        return np.asarray(feature_pts, np.float64).reshape(-1, 2)
    return np.array([p.pt if hasattr(p, "pt") else p for p in feature_pts], np.float64).reshape(-1, 2)
