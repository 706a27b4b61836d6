"""CPU reference of the relocalisation and the loop-closing SearchByProjection for fisheye (KannalaBrandt8) cameras, restated
line by line in numpy float32 / float64, with KannalaBrandt8::project by kb8_ref and the grids of projection_bounds_ref.  It
knows neither the device code nor the host twins.

A. search_by_projection_keyframe_kb8: FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th,
   ORBdist) (fmatcher.cpp:2689-2811) with a fisheye CurrentFrame (monocular, or the left camera of a two-fisheye rig: bRight
   defaults to false, so only keypoints_ and slots [0, Nleft) take part).  Per KeyFrame entry i with flags[i] & 1:
     x3Dc = Rcw * x3Dw + tcw (one gemm); uv = mpCamera->project(x3Dc); NO depth test; the closed interval over the Frame's float
     bounds; cv::norm(x3Dw - Ow) within [min, max]; PredictScale; radius = th * scale[level]; GetFeaturesInArea(u, v, r,
     level - 1, level + 1); occupied slots skipped; `dist < bestDist` from 256; bestDist <= ORBdist writes the slot, which blocks
     later entries; one rotation histogram, ComputeThreeMaxima, nmatches.
   ODDITY, NOT reproduced: the reference reads pKF->mvKeysUn[i].angle for every i < N, but a rig KeyFrame's mvKeysUn has only
   NLeft entries, so for a right-camera MapPoint (i >= NLeft) it reads past the end of the vector; the restatement reads the
   angle of mvKeysRight[i - NLeft]: kf_kps is ONE array, mvKeys followed by mvKeysRight.
   -> (nmatches, match_cur[n_cur] = KeyFrame entry or -1)

B. search_by_projection_sim3_kb8: FMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming)
   (fmatcher.cpp:750-863) for fisheye KeyFrames, ONE MapPoint list against a list of jobs that do not interact; a job is
     dict(pose=(Rcw, tcw, Ow), kps, desc (pKF's left arrays), matched (vpMatched[idx] != NULL on entry, or None),
          valid (!spAlreadyFound.count(pMP) per point, or None))
   Per job and point in ascending iMP: validity; one gemm; z < 0 rejects, z == 0 goes on; KannalaBrandt8::project;
   KeyFrame::IsInImage over the integer bounds (closed below, open above); the distance range; PO.dot(Pn) < 0.5 * dist rejects
   (both in double); PredictScale; radius = th * scale[level] (th an int); KeyFrame::GetFeaturesInArea over the left grid;
   matched keypoints skipped; level gate [level - 1, level]; `dist < bestDist` from 256; accepted on bestDist <= TH_LOW *
   ratioHamming; vpMatched[bestIdx] = pMP blocks later points; no rotation check.
   -> (match_kf: per job an array, match_kf[idx] = iMP or -1; nmatches[n_jobs]; n_gated[n_jobs] = the points that pass every
      gate up to the radius)

`census` (a dict, may be None) counts the branches taken (CENSUS).  `switches` break one rule each (SWITCHES); they are NOT the
reference and exist so that the tests can show that their cases tell the rule from its neighbour.  With "pinhole" the two
functions are projection_bounds_ref.search_by_projection_keyframe / search_by_projection_sim3, which are pinned to
oracle/orbo.py (tests/test_reloc_loop_kb8_cpu.py pins this file to both on the gate tables of tests/matcher_gate_cases.py)."""
import numpy as np

import kb8_ref as KR
from projection_bounds_ref import (HISTO, KfGrid, _dot, _gemm_row, _in_closed, _is_in_image, _norm, _predict_level, _query,
                                   _rot_bin, kf_bounds)
from undistort_ref import Grid, _three_maxima, hamming

F32 = np.float32
TH_LOW = 50
PREFIX = 8  # the default length of the sorted candidate prefix a ranking kernel keeps (vslam_tuning.sbp_topm)

CENSUS = (
    # A
    "a_flag_skip", "a_behind_inside_takes_keypoint", "a_behind_outside", "a_out_of_bounds", "a_out_of_range", "a_empty_window",
    "a_occupied_on_entry_skipped", "a_written_slot_blocks", "a_tie_first_wins", "a_above_orb_dist", "a_right_entry_matches",
    "a_right_angle_differs_from_left", "a_rotation_rejects",
    # B
    "b_invalid_point", "b_invalid_job", "b_z_negative", "b_z_zero_goes_on", "b_out_of_image", "b_u_eq_min_x_inside",
    "b_u_eq_max_x_outside", "b_below_min_distance", "b_above_max_distance", "b_viewing_angle", "b_empty_window",
    "b_matched_on_entry_skipped", "b_level_below", "b_level_above", "b_tie_across_cells", "b_tie_within_cell",
    "b_above_threshold", "b_contested_lower_imp_wins", "b_loser_moves_on", "b_prefix_runs_off_its_end")

SWITCHES = ("depth_test", "left_only_angles", "closed_upper", "level_plus", "last_tie", "z_le_0", "float_normal_dot", "pinhole")


def _note(census, name, k=1):
    if census is not None:
        census[name] = census.get(name, 0) + k


def _project_all(cam, pc, pinhole):
    """n x 3 camera points -> n x 2: KannalaBrandt8::project, or Pinhole::project (pinhole.cpp:13-16) for the pin"""
    if not pinhole:
        return KR.project(cam, pc)
    with np.errstate(all="ignore"):
        u = (F32(cam["fx"]) * pc[:, 0]) / pc[:, 2] + F32(cam["cx"])
        v = (F32(cam["fy"]) * pc[:, 1]) / pc[:, 2] + F32(cam["cy"])
    return np.stack([u, v], 1).astype(F32)


def _cell_of(grid, idx):
    for c, members in grid.cells.items():
        if idx in members:
            return c
    return None


def _better(d, best, best_i, last_tie):
    return (d <= best) if (last_tie and best_i >= 0) else (d < best)


def search_by_projection_keyframe_kb8(Tcw, Ow, cam, th, orb_dist, log_scale_factor, kf_kps, flags, x3dw, min_dist, max_dist,
                                      mp_desc, cur_kps, cur_desc, scale_factors, bounds, check_ori=True, occupied=None,
                                      gemm_double=True, n_kf_left=None, switches=(), census=None):
    """cam: a kb8_ref.camera dict (CurrentFrame.mpCamera); n_kf_left: pKF->NLeft (None: a monocular KeyFrame)"""
    unknown = set(switches) - set(SWITCHES)
    assert not unknown, unknown
    sw = set(switches)
    T = np.asarray(Tcw, F32).reshape(3, 4)
    Ow = np.asarray(Ow, F32).reshape(3)
    b = [F32(v) for v in bounds]
    n, n2 = len(kf_kps), len(cur_kps)
    nl = n if n_kf_left is None else int(n_kf_left)
    match = np.full(n2, -1, np.int32)
    entry = np.zeros(n2, np.uint8) if occupied is None else (np.asarray(occupied, np.uint8) != 0).astype(np.uint8)
    has = entry.copy()
    grid = Grid(cur_kps, bounds)
    dist = hamming(mp_desc, cur_desc) if n and n2 else None
    x3dw = np.asarray(x3dw, F32).reshape(-1, 3)
    pc = np.zeros((n, 3), F32)
    for i in range(n):
        pc[i] = [_gemm_row(T[r, :3], x3dw[i], T[r, 3], gemm_double) for r in range(3)]
    uv = _project_all(cam, pc, "pinhole" in sw) if n else np.zeros((0, 2), F32)
    rot_hist = [[] for _ in range(HISTO)]
    nm = 0
    for i in range(n):
        if not flags[i] & 1:
            _note(census, "a_flag_skip")
            continue
        behind = bool(pc[i, 2] < 0)
        if "depth_test" in sw and behind:
            continue
        u, v = F32(uv[i, 0]), F32(uv[i, 1])
        if not _in_closed(u, v, b):
            _note(census, "a_behind_outside" if behind else "a_out_of_bounds")
            continue
        d3 = _norm(x3dw[i] - Ow)
        if d3 < min_dist[i] or d3 > max_dist[i]:
            _note(census, "a_out_of_range")
            continue
        lvl = _predict_level(max_dist[i], d3, log_scale_factor, len(scale_factors))
        radius = F32(F32(th) * F32(scale_factors[lvl]))
        window = _query(grid, u, v, radius, lvl - 1, lvl + 1)
        if not window:
            _note(census, "a_empty_window")
            continue
        best, best_i, tie = 256, -1, False
        for i2 in window:
            if has[i2]:
                _note(census, "a_occupied_on_entry_skipped" if entry[i2] else "a_written_slot_blocks")
                continue
            d = int(dist[i, i2])
            if d == best and best_i >= 0:
                tie = True
            if _better(d, best, best_i, "last_tie" in sw):
                if d < best:
                    tie = False
                best, best_i = d, i2
        if best <= orb_dist:
            match[best_i] = i
            has[best_i] = 1
            nm += 1
            if tie:
                _note(census, "a_tie_first_wins")
            if behind:
                _note(census, "a_behind_inside_takes_keypoint")
            if i >= nl:
                _note(census, "a_right_entry_matches")
            if check_ori:
                angle = kf_kps["angle"][i]
                if i >= nl:
                    left = kf_kps["angle"][i - nl] if i - nl < nl else F32(0)
                    if _rot_bin(left, cur_kps["angle"][best_i]) != _rot_bin(angle, cur_kps["angle"][best_i]):
                        _note(census, "a_right_angle_differs_from_left")
                    if "left_only_angles" in sw:
                        angle = left
                rot_hist[_rot_bin(angle, cur_kps["angle"][best_i])].append(best_i)
        elif best_i >= 0:
            _note(census, "a_above_orb_dist")
    if check_ori:
        keep = _three_maxima([len(h) for h in rot_hist])
        for k in range(HISTO):
            if k not in keep:
                for i2 in rot_hist[k]:
                    match[i2] = -1
                    nm -= 1
                    _note(census, "a_rotation_rejects")
    return nm, match


def search_by_projection_sim3_kb8(jobs, points, mp_desc, cam, th, ratio_hamming, log_scale_factor, scale_factors, bounds,
                                  gemm_double=True, switches=(), census=None):
    """cam: a kb8_ref.camera dict (pKF->mpCamera; a rig KeyFrame's is the left one)"""
    unknown = set(switches) - set(SWITCHES)
    assert not unknown, unknown
    sw = set(switches)
    n = len(points)
    nlevels = len(scale_factors)
    b = kf_bounds(bounds)
    matches, nms, gated = [], np.zeros(len(jobs), np.int32), np.zeros(len(jobs), np.int32)
    for jn, job in enumerate(jobs):
        R = np.asarray(job["pose"][0], F32).reshape(3, 3)
        t = np.asarray(job["pose"][1], F32).reshape(3)
        Ow = np.asarray(job["pose"][2], F32).reshape(3)
        kps, desc = job["kps"], job["desc"]
        nk = len(kps)
        match = np.full(nk, -1, np.int32)
        entry = np.zeros(nk, np.uint8) if job.get("matched") is None else (np.asarray(job["matched"], np.uint8) != 0).astype(np.uint8)
        taken = entry.copy()
        grid = KfGrid(kps, bounds)
        dist = hamming(mp_desc, desc) if n and nk else None
        jvalid = job.get("valid")
        pc = np.zeros((n, 3), F32)
        for i in range(n):
            pc[i] = [_gemm_row(R[r], points["pos"][i], t[r], gemm_double) for r in range(3)]
        uv = _project_all(cam, pc, "pinhole" in sw) if n else np.zeros((0, 2), F32)
        nm = 0
        for i in range(n):
            mp = points[i]
            if not mp["valid"]:
                _note(census, "b_invalid_point")
                continue
            if jvalid is not None and not jvalid[i]:
                _note(census, "b_invalid_job")
                continue
            zc = pc[i, 2]
            if zc < 0.0 or ("z_le_0" in sw and zc <= 0.0):
                _note(census, "b_z_negative")
                continue
            if zc == 0.0:
                _note(census, "b_z_zero_goes_on")
            u, v = F32(uv[i, 0]), F32(uv[i, 1])
            inside = _is_in_image(u, v, b)
            if "closed_upper" in sw:
                inside = bool(u >= b[0] and u <= b[1] and v >= b[2] and v <= b[3])
            if not inside:
                _note(census, "b_out_of_image")
                if u == b[1]:
                    _note(census, "b_u_eq_max_x_outside")
                continue
            if u == b[0]:
                _note(census, "b_u_eq_min_x_inside")
            PO = np.asarray(mp["pos"], F32) - Ow
            d3 = _norm(PO)
            if d3 < mp["min_distance"]:
                _note(census, "b_below_min_distance")
                continue
            if d3 > mp["max_distance"]:
                _note(census, "b_above_max_distance")
                continue
            if "float_normal_dot" in sw:
                s = F32(0)
                for k in range(3):
                    s = F32(s + F32(PO[k] * F32(mp["normal"][k])))
                rejected = bool(s < F32(F32(0.5) * d3))
            else:
                rejected = _dot(PO, mp["normal"]) < 0.5 * float(d3)
            if rejected:
                _note(census, "b_viewing_angle")
                continue
            lvl = _predict_level(mp["max_distance"], d3, log_scale_factor, nlevels)
            radius = F32(F32(int(th)) * F32(scale_factors[lvl]))
            gated[jn] += 1
            window = _query(grid, u, v, radius, -1, -1)
            if not window:
                _note(census, "b_empty_window")
                continue
            hi = lvl + 1 if "level_plus" in sw else lvl
            best, best_i, tied = 256, -1, None
            free_best, free_i = 256, -1  # the choice of a point that meets no keypoint taken during this call
            ranked = []                  # the candidates behind the order-free gates: (distance, window position, idx)
            for pos, idx in enumerate(window):
                o = int(kps["octave"][idx])
                level_ok = not (o < lvl - 1 or o > hi)
                d = int(dist[i, idx])
                if level_ok:
                    ranked.append((min(d, 255), pos, idx))
                    if not entry[idx] and d < free_best:
                        free_best, free_i = d, idx
                if taken[idx]:
                    if entry[idx]:
                        _note(census, "b_matched_on_entry_skipped")
                    continue
                if not level_ok:
                    _note(census, "b_level_below" if o < lvl - 1 else "b_level_above")
                    continue
                if d == best and best_i >= 0 and tied is None:
                    tied = (best_i, idx)
                if _better(d, best, best_i, "last_tie" in sw):
                    if d < best:
                        tied = None
                    best, best_i = d, idx
            accepted = F32(best) <= F32(F32(TH_LOW) * F32(ratio_hamming))
            if census is not None:
                ranked.sort()
                lead = 0
                for _, _, idx in ranked:
                    if not taken[idx]:
                        break
                    lead += 1
                if lead >= PREFIX:
                    _note(census, "b_prefix_runs_off_its_end")
                if free_i >= 0 and free_i != best_i and taken[free_i] and F32(free_best) <= F32(F32(TH_LOW) * F32(ratio_hamming)):
                    _note(census, "b_contested_lower_imp_wins")
                    if accepted:
                        _note(census, "b_loser_moves_on")
            if accepted:
                taken[best_i] = 1
                match[best_i] = i
                nm += 1
                if tied is not None and census is not None:
                    _note(census, "b_tie_within_cell" if _cell_of(grid, tied[0]) == _cell_of(grid, tied[1]) else "b_tie_across_cells")
            elif best_i >= 0:
                _note(census, "b_above_threshold")
        matches.append(match)
        nms[jn] = nm
    return matches, nms, gated
