"""FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (fmatcher.cpp:546-748) with F.Nleft != -1, restated in
numpy / Python as it is written, and the rig reading of the KeyFrame-KeyFrame overload (:1100-1240).  No GPU, no native code.

F has N = Nleft + Nright features, descriptor rows and FeatureVector indices over [0, N), left first; a rig KeyFrame is indexed
the same way and features of both its sides are queries.  For a KeyFrame feature with a good MapPoint one pass over the node's
frame features skips occupied slots and keeps best / second best per side; the left write needs bestDist1 <= TH_LOW and the
ratio test; the right branch lies INSIDE `if (bestDist1 <= TH_LOW)` (:680 within :650) and its ratio test is `|| true` (:682);
one rotation histogram takes the writes of both sides.

`census` (a dict, counts are added) says which of those branches a run took; `switches` each break ONE rule, so that a test can
show that its cases notice the rule:
  right_unnested     the right branch runs outside `if (bestDist1 <= TH_LOW)`
  right_ratio        the right ratio test is enforced
  left_fail_continue a left ratio failure skips the right branch
  hist_per_side      one rotation histogram per side
  strict_th          `<` instead of `<= TH_LOW`
  right_occ_ignored  occupied right slots stay candidates
"""
import numpy as np

TH_LOW, HISTO = 50, 30
F32 = np.float32
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
SWITCHES = ("right_unnested", "right_ratio", "left_fail_continue", "hist_per_side", "strict_th", "right_occ_ignored")
CENSUS = ("left_write", "right_write", "right_after_left_ratio_fail", "right_own_ratio_refused", "right_cut_left_above_th",
          "right_cut_no_left_candidate", "occupied_best_left", "occupied_best_right")


def new_census():
    return {k: 0 for k in CENSUS}


def hamming(one, block):
    """DescriptorDistance of one descriptor to every row of block"""
    return POP[np.bitwise_xor(block, one[None, :])].sum(axis=1)


def rot_bin(a1, a2):
    rot = F32(F32(a1) - F32(a2))
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    x = float(F32(rot * (F32(1.0) / F32(HISTO))))
    b = int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))  # round(): halves away from zero
    return 0 if b == HISTO else b


def three_maxima(sizes):
    """ComputeThreeMaxima (fmatcher.cpp:2814-2857)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif max3 < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _best2(dist, idx):
    """(bestDist1, bestIdx, bestDist2) of the sequential scan over (dist, idx) in order, from 256 / -1 / 256"""
    if len(dist) == 0:
        return 256, -1, 256
    k = int(np.argmin(dist))  # the first of equal distances: `dist < bestDist1`
    d1 = int(dist[k])
    if d1 >= 256:
        return 256, -1, 256
    rest = np.delete(dist, k)
    d2 = min(int(rest.min()), 256) if len(rest) else 256
    return d1, int(idx[k]), d2


def _under(d, switches):
    return d < TH_LOW if "strict_th" in switches else d <= TH_LOW


def search_by_bow_rig(kf_kps, kf_desc, kf_flags, kf_fv, f_kps, f_desc, n_left, f_fv, nnratio=0.7, check_ori=True, switches=(),
                      census=None):
    """kf_* and f_*: keypoints (angle), descriptors (n x 32 uint8) and, for the KeyFrame, flags, left rows first; n_left =
    F.Nleft; *_fv: dicts with fv_nodes / fv_off / fv_feat.  -> (nmatches, match_f[N] = KeyFrame feature index or -1)"""
    switches = frozenset(switches)
    assert switches <= set(SWITCHES), switches
    cs = census if census is not None else new_census()
    kf_desc = np.asarray(kf_desc, np.uint8).reshape(-1, 32)
    f_desc = np.asarray(f_desc, np.uint8).reshape(-1, 32)
    N = len(f_desc)
    match = np.full(N, -1, np.int32)
    nnratio = F32(nnratio)
    kn, ko, kf = (np.asarray(kf_fv[k]) for k in ("fv_nodes", "fv_off", "fv_feat"))
    fn, fo, ff = (np.asarray(f_fv[k]) for k in ("fv_nodes", "fv_off", "fv_feat"))
    hist = [[[] for _ in range(HISTO)] for _ in range(2)]  # [side][bin]; side 1 is used by hist_per_side alone
    nm = 0
    KFit = Fit = 0
    while KFit != len(kn) and Fit != len(fn):
        if kn[KFit] == fn[Fit]:
            cand = ff[fo[Fit]:fo[Fit + 1]].astype(np.int64)
            is_left = cand < n_left
            cdesc = f_desc[cand]
            for a in range(ko[KFit], ko[KFit + 1]):
                iKF = int(kf[a])
                if not kf_flags[iKF]:
                    continue
                dist = hamming(kf_desc[iKF], cdesc)
                free = match[cand] < 0
                fl = free & is_left
                fr = (free | ("right_occ_ignored" in switches)) & ~is_left
                d1, iF, d2 = _best2(dist[fl], cand[fl])
                d1r, iFR, d2r = _best2(dist[fr], cand[fr])
                # census: an occupied candidate that would otherwise have been the side's best, near enough to be written
                for side, mask, key in ((is_left, fl, "occupied_best_left"), (~is_left, free & ~is_left, "occupied_best_right")):
                    if side.any():
                        k = int(np.argmin(np.where(side, dist, 1000)))
                        if not mask[k] and dist[k] <= TH_LOW:
                            cs[key] += 1
                right_would = _under(d1r, switches)
                left_ok = _under(d1, switches)
                if not left_ok and "right_unnested" not in switches:
                    if right_would:
                        cs["right_cut_left_above_th" if fl.any() else "right_cut_no_left_candidate"] += 1
                    continue
                ang = kf_kps["angle"][iKF]
                ratio_ok = left_ok and F32(d1) < nnratio * F32(d2)
                if ratio_ok:
                    match[iF] = iKF
                    nm += 1
                    cs["left_write"] += 1
                    if check_ori:
                        hist[0][rot_bin(ang, f_kps["angle"][iF])].append(iF)
                elif left_ok and "left_fail_continue" in switches:
                    continue
                if right_would:
                    own_ratio = F32(d1r) < nnratio * F32(d2r)
                    if "right_ratio" in switches and not own_ratio:
                        continue
                    match[iFR] = iKF
                    nm += 1
                    cs["right_write"] += 1
                    if not ratio_ok:
                        cs["right_after_left_ratio_fail"] += 1
                    if not own_ratio:
                        cs["right_own_ratio_refused"] += 1
                    if check_ori:
                        hist[1 if "hist_per_side" in switches else 0][rot_bin(ang, f_kps["angle"][iFR])].append(iFR)
            KFit += 1
            Fit += 1
        elif kn[KFit] < fn[Fit]:
            KFit = int(np.searchsorted(kn, fn[Fit], "left"))
        else:
            Fit = int(np.searchsorted(fn, kn[KFit], "left"))
    if check_ori:
        for h in hist:
            keep = three_maxima([len(b) for b in h])
            for i in range(HISTO):
                if i not in keep:
                    for idx in h[i]:
                        match[idx] = -1
                        nm -= 1
    return nm, match


def search_by_bow_keyframes_rig(kps1, desc1, flags1, n_left1, fv1, kps2, desc2, flags2, n_left2, fv2, nnratio=0.8,
                                check_ori=True):
    """FMatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (fmatcher.cpp:1100-1240) for rig KeyFrames: idx >= mvKeysUn.size() is
    skipped on both sides (:1135, :1155), and a rig's mvKeysUn has NLeft entries.  The threshold is bestDist1 < TH_LOW, the
    candidates need a good MapPoint, the result is indexed by KeyFrame 1.  -> (nmatches, match12[n1])"""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    n1, n2 = len(flags1), len(flags2)
    match12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(n2, bool)
    nnratio = F32(nnratio)
    an, ao, af = (np.asarray(fv1[k]) for k in ("fv_nodes", "fv_off", "fv_feat"))
    bn, bo, bf = (np.asarray(fv2[k]) for k in ("fv_nodes", "fv_off", "fv_feat"))
    hist = [[] for _ in range(HISTO)]
    nm = 0
    i1 = i2 = 0
    while i1 != len(an) and i2 != len(bn):
        if an[i1] == bn[i2]:
            cand = bf[bo[i2]:bo[i2 + 1]].astype(np.int64)
            for a in range(ao[i1], ao[i1 + 1]):
                idx1 = int(af[a])
                if idx1 >= n_left1 or not flags1[idx1]:
                    continue
                ok = np.array([c < n_left2 and not matched2[c] and bool(flags2[c]) for c in cand], bool)
                if not ok.any():
                    continue
                d1, best2, d2 = _best2(hamming(desc1[idx1], desc2[cand[ok]]), cand[ok])
                if d1 < TH_LOW and F32(d1) < nnratio * F32(d2):
                    match12[idx1] = best2
                    matched2[best2] = True
                    nm += 1
                    if check_ori:
                        hist[rot_bin(kps1["angle"][idx1], kps2["angle"][best2])].append(idx1)
            i1 += 1
            i2 += 1
        elif an[i1] < bn[i2]:
            i1 = int(np.searchsorted(an, bn[i2], "left"))
        else:
            i2 = int(np.searchsorted(bn, an[i1], "left"))
    if check_ori:
        keep = three_maxima([len(b) for b in hist])
        for i in range(HISTO):
            if i not in keep:
                for idx in hist[i]:
                    match12[idx] = -1
                    nm -= 1
    return nm, match12
