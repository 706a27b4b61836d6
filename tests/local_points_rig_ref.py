"""CPU reference of FMatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
(fmatcher.cpp:321-491) for both kinds of Frame, restated line by line from the reference with
Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel, bRight) (frame.cpp:678-744; undistort_ref.Grid / projection_bounds_ref._query
are that function over one keypoint set).

  rig = False   Nleft == -1: one keypoint set, the mvuRight gate (:370-375), no right branch
  rig = True    Nleft != -1 (two fisheye cameras): F.mvpMapPoints has Nleft + Nright slots, left keypoints first.  Per MapPoint
                the left branch (:339-420) and then the right branch (:422-488); each writes its own slot and, through
                mvLeftToRightMatch / mvRightToLeftMatch, the other side's slot WITHOUT looking at that slot (:409-413, :476-480).

What the state is: a slot is occupied iff it holds a MapPoint with Observations() > 0 (:366-368, :446-448).  A direct write only
lands on a free slot; a cross-write lands anywhere, so the occupancy of a slot is the Observations() > 0 of its LAST writer and
a point without observations can free a slot.  `continue` at :403-404 (left ratio test failed) leaves the loop body: the right
branch of that point is skipped.  The right radius is not multiplied by th (:425).  nmatches counts writes.

Inputs are the records of Frame::isInFrustum (orbo.MP_TRACK_DTYPE): flags bit 0 = mbTrackInView[R] with the far test
(:333) and isBad (:336) already folded in by the caller, bit 1 = Observations() > 0 (one MapPoint: the bit of either record
counts).  A right record with level == -1 takes no right branch (:424).

-> (nmatches, match[Nleft + Nright] = index of the last point written to the slot or -1, census)

`census` counts the branches taken (CENSUS names them); `broken` is a set of BREAKS, each of which breaks one rule, never what
the reference does: the tests use them to prove that their inputs can tell.
"""
import numpy as np

from projection_bounds_ref import _query
from undistort_ref import Grid, hamming

F32 = np.float32
TH_HIGH = 100

CENSUS = ("left_direct", "left_cross", "right_direct", "right_cross", "left_ratio_skips_right", "own_cross_blocks_right",
          "cross_on_occupied", "cross_frees", "freed_taken", "right_level_refused", "right_empty_window")
BREAKS = ("right_radius_th", "no_skip_right", "occupancy_kept", "own_cross_ignored", "uright_gate")


def radius_by_viewing_cos(view_cos):
    """fmatcher.cpp:493-499: the float compared with the double 0.998"""
    return F32(2.5) if float(F32(view_cos)) > 0.998 else F32(4.0)


def _best_two(cands, dist_row, octaves):
    """:355-398 / :435-468 -> bestDist, bestLevel, bestDist2, bestLevel2, bestIdx"""
    bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
    for idx in cands:
        d = int(dist_row[idx])
        if d < bd:
            bd2, bd, bl2, bl, bi = bd, d, bl, int(octaves[idx]), idx
        elif d < bd2:
            bl2, bd2 = int(octaves[idx]), d
    return bd, bl, bd2, bl2, bi


def search_by_projection_rig(track_left, track_right, mp_desc, kps_left, desc_left, kps_right, desc_right, l2r, r2l,
                             scale_factors, bounds, th=1.0, nnratio=0.8, occupied=None, mvu_right=None, rig=True, broken=()):
    broken = set(broken)
    assert broken <= set(BREAKS)
    n_mp, nl = len(track_left), len(kps_left)
    nr = len(kps_right) if rig else 0
    census = dict.fromkeys(CENSUS, 0)
    match = np.full(nl + nr, -1, np.int32)
    occ = np.zeros(nl + nr, np.uint8) if occupied is None else np.asarray(occupied, np.uint8).copy()
    assert len(occ) == nl + nr
    freed = np.zeros(nl + nr, bool)
    grid_l = Grid(kps_left, bounds)
    grid_r = Grid(kps_right, bounds) if nr else None
    dist_l = hamming(mp_desc, desc_left) if n_mp and nl else None
    dist_r = hamming(mp_desc, desc_right) if n_mp and nr else None
    th, nnratio = F32(th), F32(nnratio)
    sf = np.asarray(scale_factors, F32)
    nm = 0

    def write(slot, i, blocking, cross):
        nonlocal nm
        if cross and occ[slot]:
            census["cross_on_occupied"] += 1
            if not blocking and "occupancy_kept" not in broken:
                census["cross_frees"] += 1
                freed[slot] = True
        elif not cross and freed[slot]:
            census["freed_taken"] += 1
            freed[slot] = False
        if blocking:
            freed[slot] = False
        match[slot] = i
        if "occupancy_kept" in broken:
            occ[slot] = occ[slot] or blocking
        else:
            occ[slot] = 1 if blocking else 0
        nm += 1

    for i in range(n_mp):
        tl = track_left[i]
        tr = track_right[i] if rig else None
        in_l = bool(int(tl["flags"]) & 1)
        in_r = rig and bool(int(tr["flags"]) & 1)
        if not in_l and not in_r:
            continue
        blocking = bool((int(tl["flags"]) | (int(tr["flags"]) if rig else 0)) & 2)
        own_cross, own_cross_before = -1, 0
        if in_l:
            lvl = int(tl["level"])
            r = radius_by_viewing_cos(tl["view_cos"])
            if th != 1.0:
                r = F32(r * th)
            rs = F32(r * sf[lvl])
            cands = []
            for idx in (_query(grid_l, tl["proj_x"], tl["proj_y"], rs, lvl - 1, lvl) if nl else ()):
                if occ[idx]:
                    continue
                if (not rig or "uright_gate" in broken) and mvu_right is not None and mvu_right[idx] > 0:
                    if abs(F32(F32(tl["proj_xr"]) - F32(mvu_right[idx]))) > rs:
                        continue
                cands.append(idx)
            if cands:  # an empty vIndices and a window of occupied keypoints alike leave bestDist at 256
                bd, bl, bd2, bl2, bi = _best_two(cands, dist_l[i], kps_left["octave"])
                if bd <= TH_HIGH:
                    if bl == bl2 and F32(bd) > F32(nnratio * F32(bd2)):
                        if in_r and int(tr["level"]) != -1:
                            census["left_ratio_skips_right"] += 1
                        if "no_skip_right" not in broken:
                            continue
                    else:
                        write(bi, i, blocking, False)
                        if rig and int(l2r[bi]) != -1:
                            own_cross = int(l2r[bi]) + nl
                            own_cross_before = int(occ[own_cross])
                            write(own_cross, i, blocking, True)
                            census["left_cross"] += 1
                        else:
                            census["left_direct"] += 1
        if in_r:
            lvl = int(tr["level"])
            if lvl == -1:
                census["right_level_refused"] += 1
                continue
            r = radius_by_viewing_cos(tr["view_cos"])
            if "right_radius_th" in broken and th != 1.0:
                r = F32(r * th)
            rs = F32(r * sf[lvl])
            window = _query(grid_r, tr["proj_x"], tr["proj_y"], rs, lvl - 1, lvl) if nr else []
            if not window:
                census["right_empty_window"] += 1
                continue
            cands = []
            for idx in window:
                slot = idx + nl
                o = occ[slot]
                if slot == own_cross:
                    if o:
                        census["own_cross_blocks_right"] += 1
                    if "own_cross_ignored" in broken:
                        o = own_cross_before
                if o:
                    continue
                cands.append(idx)
            bd, bl, bd2, bl2, bi = _best_two(cands, dist_r[i], kps_right["octave"])
            if bd <= TH_HIGH:
                if bl == bl2 and F32(bd) > F32(nnratio * F32(bd2)):
                    continue
                if int(r2l[bi]) != -1:
                    write(int(r2l[bi]), i, blocking, True)
                    census["right_cross"] += 1
                else:
                    census["right_direct"] += 1
                write(bi + nl, i, blocking, False)
    return nm, match, census


def far_filtered_rig(P, track_left, track_right, depth_left):
    """fmatcher.cpp:333 in front of the matcher: mTrackDepth is the LEFT depth for every point; the device reads it as
    frame_in_frustum_rig delivers it, 0 where the left camera does not see the point, so a right-only point is never far.
    -> copies of both record arrays with bit 0 cleared on the far points"""
    tl, tr = track_left.copy(), track_right.copy()
    if P["far_points"]:
        far = np.asarray(depth_left, F32) > F32(P["th_far_points"])
        tl["flags"][far] &= np.uint32(~np.uint32(1))
        tr["flags"][far] &= np.uint32(~np.uint32(1))
    return tl, tr


def kept_indices(track_left, track_right):
    """the points that go on to the matcher, in order: left || right after the far test"""
    return np.nonzero(((track_left["flags"] | track_right["flags"]) & 1) != 0)[0]
