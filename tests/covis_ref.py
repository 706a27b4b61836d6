"""The yardstick of the covisibility mirror: the reference's observation graph and its counting loops restated in plain
Python, line by line.  File and line numbers name the reference's sources:

    mappoint.cpp   src/datastructures/mappoint.cpp    AddObservation :137-162, EraseObservation :164-197, SetBadFlag :211-234
    keyframe.cpp   src/datastructures/keyframe.cpp    TrackedMapPoints :320-339, UpdateConnections :351-444
    tracking.cpp   src/core/tracking.cpp              UpdateLocalKeyFrames :3306-3376
    localmapping.cpp  src/core/localmapping.cpp       KeyFrameCulling :946-1100

Every std::map<KeyFrame*, ..> of the reference is a dict that is WALKED IN ASCENDING order_key (the stand-in of the
pointer value), every sort of pair<int, KeyFrame*> sorts (int, order_key).  `census` counts the branches taken, so that a
case set can prove that it reaches them by this file alone."""
import collections


class Invalid(Exception):
    """what the mirror answers with VSLAM_ERR_INVALID"""


class KeyFrame:
    def __init__(self, mnId, map_id, key):
        self.mnId, self.map, self.key, self.bad = mnId, map_id, key, False


class MapPoint:
    def __init__(self, id_):
        self.id_ = id_
        self.mObservations = {}  # kf id -> [leftIndex, rightIndex]           (map<KeyFrame*, tuple<int,int>>)
        self.levels = {}         # kf id -> [octave of the left, of the right keypoint]   (read from the KeyFrame there)
        self.stereo = {}         # kf id -> !pKF->mpCamera2 && mvuRight[leftIndex] >= 0
        self.nObs = 0
        self.mbBad = False


class Graph:
    def __init__(self):
        self.kfs, self.mps = {}, {}
        self.census = collections.Counter()

    # ---------------------------------------------------------------- keyframes
    def _kf(self, kf_id):
        if kf_id not in self.kfs:
            raise Invalid("unknown keyframe %r" % kf_id)
        return self.kfs[kf_id]

    def _mp(self, mp_id):
        if mp_id not in self.mps:
            raise Invalid("unknown MapPoint %r" % mp_id)
        return self.mps[mp_id]

    def add_keyframe(self, kf_id, map_id, order_key):
        if kf_id in self.kfs or any(k.key == order_key for k in self.kfs.values()):
            raise Invalid("duplicate keyframe or order_key")
        self.kfs[kf_id] = KeyFrame(kf_id, map_id, order_key)

    def add_keyframes(self, kf_ids, map_ids, order_keys):
        kf_ids, order_keys = [int(v) for v in kf_ids], [int(v) for v in order_keys]
        if len(set(kf_ids)) != len(kf_ids) or len(set(order_keys)) != len(order_keys):
            raise Invalid("listed twice")
        live = {k.key for k in self.kfs.values()}
        if any(k in self.kfs for k in kf_ids) or any(k in live for k in order_keys):
            raise Invalid("duplicate keyframe or order_key")
        for k, m, o in zip(kf_ids, map_ids, order_keys):
            self.kfs[k] = KeyFrame(k, int(m), o)

    def set_keyframe_bad(self, kf_id):
        self._kf(kf_id).bad = True

    def set_keyframe_map(self, kf_id, map_id):
        self._kf(kf_id).map = map_id

    def erase_keyframe(self, kf_id):
        self._kf(kf_id)
        if any(kf_id in mp.mObservations for mp in self.mps.values()):
            raise Invalid("still observed")
        del self.kfs[kf_id]

    # ---------------------------------------------------------------- points
    def add_point(self, mp_id):
        if mp_id < 0 or mp_id in self.mps:
            raise Invalid("duplicate or negative MapPoint id")
        self.mps[mp_id] = MapPoint(mp_id)

    def add_observation(self, mp_id, kf_id, idx, is_right=False, level=0, stereo=False):
        """mappoint.cpp:137-162"""
        if mp_id not in self.mps or kf_id not in self.kfs or idx < 0 or not 0 <= level <= 63:
            raise Invalid("add_observation")
        mp = self.mps[mp_id]
        if kf_id in mp.mObservations:                    # :142-144
            indexes = mp.mObservations[kf_id]
        else:                                            # :145-147
            indexes = [-1, -1]
            mp.levels[kf_id] = [-1, -1]
            mp.stereo[kf_id] = False
        if is_right:                                     # :149-151  pKF->NLeft != -1 && idx >= pKF->NLeft
            indexes[1] = idx
            mp.levels[kf_id][1] = level
        else:                                            # :152-154
            indexes[0] = idx
            mp.levels[kf_id][0] = level
            mp.stereo[kf_id] = bool(stereo)
        mp.mObservations[kf_id] = indexes                # :156
        mp.nObs += 2 if stereo else 1                    # :158-161

    def _set_bad_flag(self, mp):
        """mappoint.cpp:211-220: the part that touches the graph"""
        mp.mbBad = True
        mp.mObservations, mp.levels, mp.stereo = {}, {}, {}

    def erase_observation(self, mp_id, kf_id):
        """mappoint.cpp:164-197 -> whether the point became bad"""
        mp = self._mp(mp_id)
        self._kf(kf_id)
        bBad = False
        if kf_id in mp.mObservations:                    # :169
            leftIndex, rightIndex = mp.mObservations[kf_id]
            if leftIndex != -1:                          # :174-179
                mp.nObs -= 2 if mp.stereo[kf_id] else 1
            if rightIndex != -1:                         # :180-182
                mp.nObs -= 1
            del mp.mObservations[kf_id]                  # :184
            del mp.levels[kf_id]
            del mp.stereo[kf_id]
            if mp.nObs <= 2:                             # :190-191
                bBad = True
        if bBad:                                         # :195-196
            self._set_bad_flag(mp)
        return bBad

    def clear_point(self, mp_id):
        """the first block of SetBadFlag (:213-220) and of Replace (:250-259)"""
        self._set_bad_flag(self._mp(mp_id))

    def erase_point(self, mp_id):
        self._mp(mp_id)
        del self.mps[mp_id]

    def clear_map(self, map_id):
        """the keyframes of the map go, and with them every MapPoint that one of them observes"""
        gone = {k for k, kf in self.kfs.items() if kf.map == map_id}
        for m in [m for m, mp in self.mps.items() if any(k in gone for k in mp.mObservations)]:
            del self.mps[m]
        for k in gone:
            del self.kfs[k]

    def clear(self):
        self.kfs, self.mps = {}, {}

    def size(self):
        return len(self.kfs), len(self.mps), sum(len(mp.mObservations) for mp in self.mps.values())

    def _ordered(self, kf_ids):
        """a std::map<KeyFrame*, ..> is walked in ascending pointer = order_key"""
        return sorted(kf_ids, key=lambda k: self.kfs[k].key)

    def get_point(self, mp_id):
        """-> (nObs, bad, [(kf_id, left_idx, right_idx, left_level, right_level, stereo)] in ascending order_key)"""
        mp = self._mp(mp_id)
        return mp.nObs, mp.mbBad, [(k, mp.mObservations[k][0], mp.mObservations[k][1], mp.levels[k][0], mp.levels[k][1],
                                    int(mp.stereo[k])) for k in self._ordered(mp.mObservations)]

    # ---------------------------------------------------------------- queries
    def _job_error(self, mp_ids, kf_id, need_kf):
        err = 0
        if any(m is not None and m != -1 and m not in self.mps for m in mp_ids):
            err |= 1
        if need_kf and kf_id not in self.kfs:
            err |= 2
        return err

    def tracked_map_points(self, mp_ids, minObs):
        """keyframe.cpp:320-339"""
        nPoints = 0
        bCheckObs = minObs > 0                           # :324
        for m in mp_ids:                                 # :325
            if m is None or m == -1:                     # :327
                continue
            pMP = self.mps[m]
            if not pMP.mbBad:                            # :328
                if bCheckObs:                            # :329
                    if pMP.nObs >= minObs:               # :330
                        nPoints += 1
                else:
                    nPoints += 1                         # :333
        return nPoints

    def connections(self, job):
        """job: dict(mode, self_kf, map_id, min_obs, mp_ids) -> dict like V.CovisibilityMap.connections delivers"""
        mode, mp_ids = job.get("mode", 0), list(job["mp_ids"])
        C = self.census
        empty = dict(counter_kf=[], counter_n=[], kf_max=-1, n_max=0, ordered_kf=[], ordered_w=[], n_tracked=0)
        err = self._job_error(mp_ids, job.get("self_kf", -1), mode == 0)
        if err:
            return dict(empty, error=err)
        out = self._update_connections(job, mp_ids) if mode == 0 else self._vote(mp_ids)
        out["n_tracked"] = self.tracked_map_points(mp_ids, job.get("min_obs", 0))
        out["error"] = 0
        C["mode.%d" % mode] += 1
        return out

    def _update_connections(self, job, mp_ids):
        """keyframe.cpp:351-444 up to :427"""
        C, mnId, mpMap = self.census, job["self_kf"], job["map_id"]
        KFcounter = collections.Counter()                # map<KeyFrame*, int>
        seen = set()
        for m in mp_ids:                                 # :363
            if m is None or m == -1:                     # :367
                C["conn.null_point"] += 1
                continue
            pMP = self.mps[m]
            if pMP.mbBad:                                # :370
                C["conn.bad_point"] += 1
                continue
            if m in seen:
                C["conn.point_listed_twice"] += 1
            seen.add(m)
            for k in self._ordered(pMP.mObservations):   # :375
                kf = self.kfs[k]
                if kf.mnId == mnId:                      # :377
                    C["conn.observer_self"] += 1
                    continue
                if kf.bad:
                    C["conn.observer_bad"] += 1
                    continue
                if kf.map != mpMap:
                    C["conn.observer_other_map"] += 1
                    continue
                KFcounter[k] += 1                        # :379
        out = dict(counter_kf=self._ordered(KFcounter), kf_max=-1, n_max=0, ordered_kf=[], ordered_w=[])
        out["counter_n"] = [KFcounter[k] for k in out["counter_kf"]]
        if not KFcounter:                                # :385
            C["conn.empty_counter"] += 1
            return out
        nmax, pKFmax, th = 0, None, 15                   # :390-392
        vPairs = []
        for k in self._ordered(KFcounter):               # :398
            n = KFcounter[k]
            if n == nmax:
                C["conn.tie_for_nmax"] += 1
            if n > nmax:                                 # :402
                nmax, pKFmax = n, k
            if n == th:
                C["conn.count_eq_15"] += 1
            if n == th - 1:
                C["conn.count_eq_14"] += 1
            if n >= th:                                  # :407
                vPairs.append((n, self.kfs[k].key, k))
        if not vPairs:                                   # :414
            C["conn.fallback_single"] += 1
            vPairs.append((nmax, self.kfs[pKFmax].key, pKFmax))
        else:
            C["conn.th15_path"] += 1
        vPairs.sort()                                    # :420  pair<int, KeyFrame*>: by count, then pointer
        if len({p[0] for p in vPairs}) < len(vPairs):
            C["conn.equal_weights_in_ordered"] += 1
        lKFs, lWs = [], []
        for n, _, k in vPairs:                           # :423-427 push_front
            lKFs.insert(0, k)
            lWs.insert(0, n)
        out.update(kf_max=pKFmax, n_max=nmax, ordered_kf=lKFs, ordered_w=lWs)
        return out

    def _vote(self, mp_ids):
        """tracking.cpp:3309-3376"""
        C = self.census
        keyframeCounter = collections.Counter()
        for m in mp_ids:                                 # :3312
            if m is None or m == -1:                     # :3315
                continue
            pMP = self.mps[m]
            if not pMP.mbBad:                            # :3317
                for k in self._ordered(pMP.mObservations):   # :3320
                    keyframeCounter[k] += 1              # :3321
            else:
                C["vote.bad_point"] += 1                 # :3325 (the caller's NULL write)
        mx, pKFmax = 0, -1                               # :3354-3355
        kfs, ns = [], []
        for k in self._ordered(keyframeCounter):         # :3361
            if self.kfs[k].bad:                          # :3365
                C["vote.bad_keyframe"] += 1
                continue
            if keyframeCounter[k] > mx:                  # :3368
                mx, pKFmax = keyframeCounter[k], k
            kfs.append(k)                                # :3374
            ns.append(keyframeCounter[k])
        return dict(counter_kf=kfs, counter_n=ns, kf_max=pKFmax, n_max=mx, ordered_kf=[], ordered_w=[])

    def culling(self, job, th_obs=3):
        """localmapping.cpp:990-1052 for one keyframe: job = dict(kf_id, mp_ids, levels); mp_ids[i] is None / -1 for a NULL
        point and for one the depth gate :1003-1007 rejects -> dict(error, n_mps, n_redundant)"""
        C, mp_ids = self.census, list(job["mp_ids"])
        err = self._job_error(mp_ids, job["kf_id"], True)
        if err:
            return dict(error=err, n_mps=0, n_redundant=0)
        pKF = job["kf_id"]
        thObs = th_obs                                   # :992-993
        nRedundantObservations, nMPs = 0, 0              # :994-995
        for i, m in enumerate(mp_ids):                   # :996
            if m is None or m == -1:                     # :999, :1003-1007
                continue
            pMP = self.mps[m]
            if pMP.mbBad:                                # :1001
                C["cull.bad_point"] += 1
                continue
            nMPs += 1                                    # :1009
            if pMP.nObs == thObs:
                C["cull.nobs_eq_3"] += 1
            if pMP.nObs == thObs + 1:
                C["cull.nobs_eq_4"] += 1
            if pMP.nObs > thObs:                         # :1010
                if len(pMP.mObservations) == 2:
                    C["cull.stereo_lifts_two_keyframes"] += 1
                scaleLevel = job["levels"][i]            # :1012-1014
                nObs = 0                                 # :1016
                for k in self._ordered(pMP.mObservations):   # :1017
                    if k == pKF:                         # :1020
                        continue
                    leftIndex, rightIndex = pMP.mObservations[k]
                    scaleLeveli = -1                     # :1024
                    if leftIndex != -1:                  # :1025-1030 (NLeft == -1: the left index is the only one)
                        scaleLeveli = pMP.levels[k][0]
                    if rightIndex != -1:                 # :1031-1035
                        rightLevel = pMP.levels[k][1]
                        if leftIndex == -1:
                            C["cull.rig_right_only"] += 1
                        elif scaleLeveli > rightLevel:
                            C["cull.rig_both_right_smaller"] += 1
                        else:
                            C["cull.rig_both_left_smaller_or_equal"] += 1
                        scaleLeveli = rightLevel if (scaleLeveli == -1 or scaleLeveli > rightLevel) else scaleLeveli
                    else:
                        C["cull.left_only"] += 1
                    if scaleLeveli == scaleLevel + 1:
                        C["cull.level_eq_plus_1"] += 1
                    if scaleLeveli == scaleLevel + 2:
                        C["cull.level_eq_plus_2"] += 1
                    if scaleLeveli <= scaleLevel + 1:    # :1038
                        nObs += 1                        # :1040
                        if nObs > thObs:                 # :1041-1042
                            break
                if nObs == thObs:
                    C["cull.qualifying_eq_3"] += 1
                if nObs == thObs + 1:
                    C["cull.qualifying_eq_4"] += 1
                if nObs > thObs:                         # :1045
                    nRedundantObservations += 1          # :1047
        return dict(error=0, n_mps=nMPs, n_redundant=nRedundantObservations)


def keyframe_set_bad_flag(target, kf_id, mp_ids):
    """KeyFrame::SetBadFlag (keyframe.cpp:530-629) as far as the graph goes: every MapPoint of the keyframe loses the
    observation (:553 pMP->EraseObservation(this)), then mbBad (:629).  `target` is a Graph or a mirror."""
    for m in mp_ids:
        if m is not None and m != -1:
            target.erase_observation(m, kf_id)
    target.set_keyframe_bad(kf_id)
