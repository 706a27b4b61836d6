"""CPU reference of FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) for a two-fisheye rig
(fmatcher.cpp:2494-2684 with CurrentFrame.Nleft != -1), restated line by line, with Frame::GetFeaturesInArea(x, y, r, minLevel,
maxLevel, bRight) as projection_bounds_ref._query over the keypoint set of one side.

Per query i = 0 .. LastFrame.N - 1 (LastFrame.N = Nleft + Nright; octave and angle from keypoints_[i] or
keypointsRight_[i - Nleft], which the caller passes as ONE array):

  left    x3Dc = Rcw * x3Dw + tcw (one gemm); invzc = 1.0 / z in double, rounded: invzc < 0 -> continue;
          uv = mpCamera->project(x3Dc) (KannalaBrandt8); outside the closed grid bounds -> continue;
          window over keypoints_ with the forward / backward / +-1 level rule; EMPTY -> continue (:2534-2535);
          no mvuRight gate in a rig (:2550); best <= TH_HIGH writes slot bestIdx2
  right   (:2593-2658, reached unless the left branch left by a `continue`; a left window of occupied candidates falls through)
          x3Dr = Rrl * x3Dc + trl (one gemm); uv = CurrentFrame.mpCamera->project(x3Dr): the LEFT camera's model; NO depth test,
          NO in-frame test, NO empty-window continue; window over keypointsRight_, same radius and level rule; occupancy,
          descriptor and the write at i2 + Nleft
  state   a slot is occupied iff it holds a MapPoint with Observations() > 0; a match by a point without observations leaves
          the slot free: a later query may overwrite it (last writer stays, two histogram entries, nmatches counts both)
  finish  ONE rotation histogram over both sides, ComputeThreeMaxima once; every entry of a rejected bin clears its slot and
          decrements nmatches.  mvLeftToRightMatch / mvRightToLeftMatch are not read.

-> (nmatches, match[Nleft + Nright] = index i of the last-frame entry in the slot or -1, census)

`project(cam, x, y, z) -> (u, v)` is a parameter (default KannalaBrandt8::project by kb8_ref): with Pinhole::project, no right
keypoints and no mvuRight the function is projection_bounds_ref.search_by_projection_frame, which is pinned to oracle/orbo.py
(tests/test_frame_projection_rig_cpu.py pins this file to it).

`census` counts the branches taken (CENSUS).  The "would match" entries evaluate the skipped right branch on the side, against
the occupancy of that moment, without writing.  `per_side_hist=True` is NOT the reference: it runs ComputeThreeMaxima once per
side, which the tests use to show that their histogram case can tell.

right_behind_camera: x3Dr.z < 0 and a non-empty right window.  With kb8_cases.LOCAL_CAM (f = 118 px, image 320 x 240) a point
behind the camera has theta > pi / 2 and lands more than 185 px from the principal point, i.e. outside the image except towards
its corners; the window (radius th * scale) still reaches keypoints near the border, so the entry is taken
(frame_projection_rig_cases.py: "right_behind").
"""
import numpy as np

import kb8_ref as KR
from projection_bounds_ref import HISTO, _gemm_row, _in_closed, _query, _rot_bin
from undistort_ref import Grid, _three_maxima, hamming

F32 = np.float32
TH_HIGH = 100

CENSUS = ("left_invz_skips_right", "left_out_of_frame_skips_right", "left_empty_window_skips_right",
          "left_all_occupied_right_matches", "right_uv_outside_bounds_matches", "right_behind_camera",
          "overwrite_without_observations", "joint_histogram_rejects", "last_octave_from_right_array", "same_point_both_slots",
          "forward", "backward", "neither", "left_match", "right_match", "right_empty_window")


def kb8_project(cam, x, y, z):
    uv = KR.project(cam, np.array([[x, y, z]], F32))
    return F32(uv[0, 0]), F32(uv[0, 1])


def pinhole_project(cam, x, y, z):
    """Pinhole::project (pinhole.cpp:13-16)"""
    with np.errstate(all="ignore"):
        return (F32(F32(F32(cam["fx"]) * x) / z + F32(cam["cx"])), F32(F32(F32(cam["fy"]) * y) / z + F32(cam["cy"])))


def search_by_projection_frame_rig(Tcw, Trl, cam, th, last_kps, flags, x3dw, mp_desc, kps_left, desc_left, kps_right,
                                   desc_right, scale_factors, bounds, forward=False, backward=False, check_ori=True,
                                   occupied=None, gemm_double=True, project=kb8_project, n_last_left=None,
                                   per_side_hist=False):
    T = np.asarray(Tcw, F32).reshape(3, 4)
    Trl = np.asarray(Trl, F32).reshape(3, 4)
    b = [F32(v) for v in bounds]
    n_last, nl, nr = len(last_kps), len(kps_left), len(kps_right)
    nll = n_last if n_last_left is None else n_last_left  # LastFrame.Nleft, for the census alone
    census = dict.fromkeys(CENSUS, 0)
    match = np.full(nl + nr, -1, np.int32)
    occ = np.zeros(nl + nr, np.uint8) if occupied is None else np.asarray(occupied, np.uint8).copy()
    assert len(occ) == nl + nr
    grid_l, grid_r = Grid(kps_left, bounds), Grid(kps_right, bounds)
    dist_l = hamming(mp_desc, desc_left) if n_last and nl else None
    dist_r = hamming(mp_desc, desc_right) if n_last and nr else None
    sf = np.asarray(scale_factors, F32)
    rot_hist = [[] for _ in range(HISTO)]
    matched = np.zeros(n_last, np.uint8)  # bit 0: the left branch of i wrote, bit 1: the right one
    nm = 0

    def best_of(window, dist_row, base):
        best, best_i = 256, -1
        for i2 in window:
            if occ[i2 + base]:
                continue
            if dist_row[i2] < best:
                best, best_i = int(dist_row[i2]), i2
        return best, best_i

    def right_branch(i, xc, radius, lv):
        """-> (window, uv, z of x3Dr, bestDist, bestIdx2) of :2594-2634, nothing written"""
        xr = [_gemm_row(Trl[r, :3], xc, Trl[r, 3], gemm_double) for r in range(3)]
        u, v = project(cam, *xr)
        window = _query(grid_r, u, v, radius, *lv) if nr else []
        best, best_i = best_of(window, dist_r[i], nl) if window else (256, -1)
        return window, (u, v), xr[2], best, best_i

    def write(slot, i, kp_angle):
        nonlocal nm
        if match[slot] != -1:
            census["overwrite_without_observations"] += 1  # an occupied slot is never a candidate
        match[slot] = i
        occ[slot] = 1 if flags[i] & 2 else 0
        nm += 1
        if check_ori:
            rot_hist[_rot_bin(last_kps["angle"][i], kp_angle)].append(slot)

    for i in range(n_last):
        if not flags[i] & 1:
            continue
        xc = [_gemm_row(T[r, :3], x3dw[i], T[r, 3], gemm_double) for r in range(3)]
        o = int(last_kps["octave"][i])
        radius = F32(F32(th) * sf[o])
        lv = (o, -1) if forward else (0, o) if backward else (o - 1, o + 1)

        def skipped(name):
            if right_branch(i, xc, radius, lv)[3] <= TH_HIGH:
                census[name] += 1

        with np.errstate(all="ignore"):
            invzc = F32(np.float64(1.0) / np.float64(xc[2]))
        if invzc < 0:
            skipped("left_invz_skips_right")
            continue
        u, v = project(cam, *xc)
        if not _in_closed(u, v, b):
            skipped("left_out_of_frame_skips_right")
            continue
        window = _query(grid_l, u, v, radius, *lv) if nl else []
        if not window:
            skipped("left_empty_window_skips_right")
            continue
        census["forward" if forward else "backward" if backward else "neither"] += 1
        if i >= nll and i - nll < nll and int(last_kps["octave"][i - nll]) != o:
            census["last_octave_from_right_array"] += 1
        best, best_i = best_of(window, dist_l[i], 0)
        if best <= TH_HIGH:
            write(best_i, i, kps_left["angle"][best_i])
            census["left_match"] += 1
            matched[i] |= 1
        rwin, (ur, vr), zr, rbest, rbest_i = right_branch(i, xc, radius, lv)
        if not rwin:
            census["right_empty_window"] += 1
        elif zr < 0:
            census["right_behind_camera"] += 1
        if rbest <= TH_HIGH:
            if best_i < 0:
                census["left_all_occupied_right_matches"] += 1
            if not _in_closed(ur, vr, b):
                census["right_uv_outside_bounds_matches"] += 1
            write(rbest_i + nl, i, kps_right["angle"][rbest_i])
            census["right_match"] += 1
            matched[i] |= 2

    # the same MapPoint in a left and a right slot of the last frame: two queries with one position and one descriptor
    def ident(i):
        return np.asarray(x3dw[i], F32).tobytes() + np.asarray(mp_desc[i], np.uint8).tobytes()

    in_left = {ident(i) for i in range(min(nll, n_last)) if matched[i]}
    census["same_point_both_slots"] = sum(1 for j in range(nll, n_last) if matched[j] and ident(j) in in_left)

    if check_ori:
        joint = _three_maxima([len(h) for h in rot_hist])
        keep_l = _three_maxima([sum(1 for s in h if s < nl) for h in rot_hist])
        keep_r = _three_maxima([sum(1 for s in h if s >= nl) for h in rot_hist])
        for k in range(HISTO):
            for slot in rot_hist[k]:
                side_keeps = k in (keep_l if slot < nl else keep_r)
                if k not in joint and side_keeps:
                    census["joint_histogram_rejects"] += 1
                if (not side_keeps) if per_side_hist else (k not in joint):
                    match[slot] = -1
                    nm -= 1
    return nm, match, census
