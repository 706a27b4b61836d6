"""CPU reference of the search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame and both cameras of a
two-fisheye rig (fmatcher.cpp:1918-2119 with pKF->NLeft != -1; keyframe.cpp:656-703) and of Fuse(pKF, Scw, ..) (:2121-2243,
sim3), restated line by line in numpy float32 / float64, with KannalaBrandt8::project by kb8_ref and the KeyFrame grid of
projection_bounds_ref (KfGrid: the Frame's cells and inverses, the window origin and IsInImage over the KeyFrame's int bounds).

One list of MapPoints against a list of jobs; a job is one call of Fuse: one camera of one KeyFrame,
  dict(pose=(Rcw, tcw, Ow) of THAT camera, camera=0 | 1, sim3=bool, kps, desc (the side's own arrays), idx_offset (0, or NLeft
       for bRight), valid (one byte per MapPoint: !IsInKeyFrame(pKF), or None), left_pose (only read by a switch))

Per job and MapPoint:
  valid        points[i].valid (pMP && !isBad()) and the job's valid[i]
  gates        p3Dc = Rcw * p3Dw + tcw (one gemm); z < 0 rejects, z == 0 goes on; uv = pCamera->project with the JOB'S camera
               (mpCamera2 for bRight); KeyFrame::IsInImage (closed below, open above); cv::norm(p3Dw - Ow) within [min, max];
               PO.dot(Pn) < 0.5 * dist3D rejects (both in double); PredictScale; radius th * scale[level]
  window       GetFeaturesInArea(u, v, r, bRight) over the side's grid: columns outer, rows inner, ascending index in a cell;
               level gate [level - 1, level]
  chi2         a rig's mvuRight is -1 throughout: e2 * invSigma2[kpLevel] > 5.99 rejects (the right call's read of
               mvuRight[right-local idx], past the end where idx >= Nleft, is NOT reproduced); none with sim3
  best         `dist < bestDist` from 256 (sim3: INT_MAX): the first of the window order wins a tie; 256 never wins without sim3
  report       local index + idx_offset; nothing: -1 / 256

-> (best_idx[n_jobs, n], best_dist[n_jobs, n])

`census` (a dict, may be None) counts the branches taken (CENSUS).  `switches` break one rule each (SWITCHES); they are NOT the
reference and exist so that the tests can show that their cases tell the rule from its neighbour.  With the "pinhole" switch,
camera 0 and idx_offset 0 the function is projection_bounds_ref.fuse_search / orbo.fuse_search with mvuRight = -1
(tests/test_fuse_rig_cpu.py pins that on the gate tables of tests/matcher_gate_cases.py)."""
import numpy as np

import kb8_ref as KR
from projection_bounds_ref import KfGrid, _dot, _gemm_row, _is_in_image, _norm, _predict_level, _query, kf_bounds
from undistort_ref import hamming

F32 = np.float32
TH_LOW = 50
INT_MAX = 2**31 - 1

CENSUS = ("invalid_point", "invalid_job", "z_negative", "z_zero_goes_on", "out_left", "out_right", "out_top", "out_bottom",
          "u_eq_min_x_inside", "u_eq_max_x_outside", "below_min_distance", "above_max_distance", "viewing_angle",
          "empty_window", "level_below", "level_above", "chi2_reject", "tie_across_cells", "tie_within_cell",
          "best_above_th_low", "offset_applied", "sim3_far")

SWITCHES = ("right_through_cam0", "right_left_pose", "no_offset", "chi2_7_8", "last_tie", "level_plus", "z_le_0", "pinhole")


def _project_all(cam, pc, pinhole):
    """n x 3 camera points -> n x 2"""
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


def fuse_search_rig(jobs, points, mp_desc, cams, th, log_scale_factor, scale_factors, inv_sigma2, bounds, gemm_double=True,
                    switches=(), census=None):
    """cams = (mpCamera, mpCamera2) as kb8_ref.camera dicts (cams[1] may be None when no job has camera 1)"""
    unknown = set(switches) - set(SWITCHES)
    assert not unknown, unknown
    sw = set(switches)
    n = len(points)
    nlevels = len(scale_factors)
    b = kf_bounds(bounds)
    bi = np.full((len(jobs), n), -1, np.int32)
    bd = np.full((len(jobs), n), 256, np.int32)

    def note(name):
        if census is not None:
            census[name] = census.get(name, 0) + 1

    for jn, job in enumerate(jobs):
        cam_i, sim3 = int(job["camera"]), bool(job["sim3"])
        assert not (sim3 and cam_i)
        pose = job["pose"]
        if cam_i == 1 and "right_left_pose" in sw:
            pose = job["left_pose"]
        R = np.asarray(pose[0], F32).reshape(3, 3)
        t = np.asarray(pose[1], F32).reshape(3)
        Ow = np.asarray(pose[2], F32).reshape(3)
        cam = cams[0] if (cam_i == 0 or "right_through_cam0" in sw) else cams[1]
        kps, desc = job["kps"], job["desc"]
        off = 0 if "no_offset" in sw else int(job["idx_offset"])
        grid = KfGrid(kps, bounds)
        dist = hamming(mp_desc, desc) if n and len(kps) else None
        jvalid = job.get("valid")
        # the gemm and the projection of every candidate point at once (elementwise the same operations)
        pc = np.zeros((n, 3), F32)
        for i in range(n):
            pc[i] = [_gemm_row(R[r], points["pos"][i], t[r], gemm_double) for r in range(3)]
        uv = _project_all(cam, pc, "pinhole" in sw)
        for i in range(n):
            mp = points[i]
            if not mp["valid"]:
                note("invalid_point")
                continue
            if jvalid is not None and not jvalid[i]:
                note("invalid_job")
                continue
            zc = pc[i, 2]
            if zc < 0.0 or ("z_le_0" in sw and zc <= 0.0):
                note("z_negative")
                continue
            if zc == 0.0:
                note("z_zero_goes_on")
            u, v = F32(uv[i, 0]), F32(uv[i, 1])
            if not _is_in_image(u, v, b):
                if u < b[0]:
                    note("out_left")
                elif u >= b[1]:
                    note("out_right")
                    if u == b[1]:
                        note("u_eq_max_x_outside")
                elif v < b[2]:
                    note("out_top")
                elif v >= b[3]:
                    note("out_bottom")
                continue
            if u == b[0]:
                note("u_eq_min_x_inside")
            PO = np.asarray(mp["pos"], F32) - Ow
            d3 = _norm(PO)
            if d3 < mp["min_distance"]:
                note("below_min_distance")
                continue
            if d3 > mp["max_distance"]:
                note("above_max_distance")
                continue
            if _dot(PO, mp["normal"]) < 0.5 * float(d3):
                note("viewing_angle")
                continue
            lvl = _predict_level(mp["max_distance"], d3, log_scale_factor, nlevels)
            radius = F32(F32(th) * F32(scale_factors[lvl]))
            window = _query(grid, u, v, radius, -1, -1)
            if not window:
                note("empty_window")
                continue
            best, best_i, tied = (INT_MAX if sim3 else 256), -1, None
            hi = lvl + 1 if "level_plus" in sw else lvl
            for idx in window:
                o = int(kps["octave"][idx])
                if o < lvl - 1:
                    note("level_below")
                    continue
                if o > hi:
                    note("level_above")
                    continue
                if not sim3:
                    ex, ey = F32(u - kps["x"][idx]), F32(v - kps["y"][idx])
                    e2 = F32(F32(ex * ex) + F32(ey * ey))
                    chi2 = F32(e2 * F32(inv_sigma2[o]))
                    if float(chi2) > (7.8 if "chi2_7_8" in sw else 5.99):
                        note("chi2_reject")
                        continue
                d = int(dist[i, idx])
                if d == best and best_i >= 0 and tied is None:
                    tied = (best_i, idx)  # the holder of the best distance and the first candidate that equals it
                if (d <= best) if ("last_tie" in sw and best_i >= 0) else (d < best):
                    if d < best:
                        tied = None
                    best, best_i = d, idx
            if best_i < 0:
                continue
            if tied is not None and census is not None:
                ca, cb = _cell_of(grid, tied[0]), _cell_of(grid, tied[1])
                note("tie_within_cell" if ca == cb else "tie_across_cells")
            if best > TH_LOW:
                note("best_above_th_low")
            if sim3 and best >= 256:
                note("sim3_far")
            if off:
                note("offset_applied")
            bi[jn, i], bd[jn, i] = best_i + off, min(best, 256)
    return bi, bd
