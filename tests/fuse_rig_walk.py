"""A toy map for the walk that follows the rig Fuse search (LocalMapping::SearchInNeighbors, localmapping.cpp:776-810): MapPoints
with observations, KeyFrames with MapPoint slots, MapPoint::Replace (mappoint.cpp:243-295) and a deterministic stand-in for
ComputeDistinctiveDescriptors -- the survivor of a Replace takes the descriptor of the point it replaced.

sequential(..)  the reference: for every job (one call of Fuse: one camera of one KeyFrame), for every point, search and mutate
                interleaved (fmatcher.cpp:1953-2116)
batch_walk(..)  ONE search of all (job, point) pairs over the map as it is at the start, then the walk of INTEGRATION.md ("Fuse
                for a rig"), which include/vslam_shim.hpp implements as FuseWalk: jobs in call order, points in order; at each
                pair skip when isBad() or IsInKeyFrame(pKF) holds NOW; a MapPoint whose descriptor was recomputed earlier in the
                walk gets its remaining searches redone, one point each (`stale_rule=False` leaves that out: NOT the rule)
Both take search(job_indices, point_ids) -> (best_idx, best_dist) arrays [len(job_indices), len(point_ids)] evaluated with the
map's CURRENT descriptors and validity."""
import copy

import numpy as np

TH_LOW = 50


class ToyMap:
    def __init__(self, n_left):
        self.n_left = n_left          # per KeyFrame: NLeft
        self.desc = {}                # MapPoint id -> descriptor
        self.bad = {}
        self.obs = {}                 # MapPoint id -> {kf: [left index, right index]}
        self.slots = {kf: {} for kf in n_left}  # kf -> {index: MapPoint id}
        self.recomputed = set()
        self.log = []

    def add_point(self, pid, desc):
        self.desc[pid], self.bad[pid], self.obs[pid] = np.asarray(desc, np.uint8).copy(), False, {}

    def observations(self, pid):
        return sum(1 for lr in self.obs[pid].values() for v in lr if v != -1)

    def in_keyframe(self, pid, kf):
        return kf in self.obs[pid]

    def add_observation(self, pid, kf, idx):
        lr = self.obs[pid].setdefault(kf, [-1, -1])
        lr[0 if idx < self.n_left[kf] else 1] = idx

    def replace(self, this, by):
        """MapPoint `this`->Replace(`by`)"""
        if this == by:
            return
        obs, self.obs[this], self.bad[this] = self.obs[this], {}, True
        for kf, lr in obs.items():
            if not self.in_keyframe(by, kf):
                for idx in lr:
                    if idx != -1:
                        self.slots[kf][idx] = by
                        self.add_observation(by, kf, idx)
            else:
                for idx in lr:
                    if idx != -1:
                        self.slots[kf].pop(idx, None)
        self.desc[by] = self.desc[this].copy()  # the stand-in for ComputeDistinctiveDescriptors
        self.recomputed.add(by)

    def fuse(self, pid, kf, best_idx, best_dist):
        """fmatcher.cpp:2093-2112"""
        if best_dist > TH_LOW:
            return
        in_kf = self.slots[kf].get(best_idx)
        if in_kf is not None:
            if not self.bad[in_kf]:
                if self.observations(in_kf) > self.observations(pid):
                    self.replace(pid, in_kf)
                else:
                    self.replace(in_kf, pid)
        else:
            self.add_observation(pid, kf, best_idx)
            self.slots[kf][best_idx] = pid
        self.log.append((pid, kf, int(best_idx)))

    def state(self):
        return (sorted((k, sorted(v.items())) for k, v in self.slots.items()), sorted(self.bad.items()),
                sorted((p, d.tobytes()) for p, d in self.desc.items()), self.log)


def sequential(m, job_kf, points, search):
    m = copy.deepcopy(m)
    for j, kf in enumerate(job_kf):
        for pid in points:
            if m.bad[pid] or m.in_keyframe(pid, kf):
                continue
            bi, bd = search(m, [j], [pid])
            if bi[0, 0] >= 0:
                m.fuse(pid, kf, bi[0, 0], bd[0, 0])
    return m


def batch_walk(m, job_kf, points, search, stale_rule=True):
    """-> (the map after the walk, number of one-point searches redone)"""
    m = copy.deepcopy(m)
    bi, bd = search(m, list(range(len(job_kf))), list(points))
    redone = 0
    for j, kf in enumerate(job_kf):
        for k, pid in enumerate(points):
            if m.bad[pid] or m.in_keyframe(pid, kf):
                continue
            i, d = bi[j, k], bd[j, k]
            if stale_rule and pid in m.recomputed:
                one_i, one_d = search(m, [j], [pid])
                i, d = one_i[0, 0], one_d[0, 0]
                redone += 1
            if i >= 0:
                m.fuse(pid, kf, i, d)
    return m, redone
