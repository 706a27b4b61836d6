/* vslam_fuse_rank_body.inc -- the second half of one MapPoint's search in k_fuse_rank and k_fuse_rank_rig
 * (vslam_projection_kernels.hip), included in the per-point loop of both: the window of KeyFrame::GetFeaturesInArea, the level
 * gate, the chi2 gate, the Hamming minimum with its key, the `far` rule of the Scw overload, the wave reduction and the write.
 * In scope at the include: go, u, v, radius, level, kbnd, inv, cand, lane, q, best, far, A (mpDesc, invSigma2, nlevels); in
 * k_fuse_rank also ur.  The includer defines, and undefines afterwards:
 *   FUSE_NKF        keypoints of the KeyFrame side          FUSE_KF_DESC    their descriptor rows
 *   FUSE_SIM3       0 / 1 / 2 as in vslam_fuse_params       FUSE_RIG        1: mvuRight is -1 throughout (no stereo chi2 branch)
 *   FUSE_OFFSET     added to a reported index               FUSE_BEST_IDX / FUSE_BEST_DIST   the output rows */
        if (go) {
            const SiWindow win = si_window_b(u, v, radius, kbnd, inv);
            if (!win.empty) {
                const uint4 da = ((const uint4*)A.mpDesc)[(size_t)q * 2], db = ((const uint4*)A.mpDesc)[(size_t)q * 2 + 1];
                for (int c = lane; c < FUSE_NKF; c += 64) {
                    const SbpCand cd = cand[c];
                    if (cd.cell == 0xFFFF || !si_in_window(cd, win, u, v, radius)) continue;
                    const int kpLevel = cd.octave;
                    if (kpLevel < level - 1 || kpLevel > level) continue;
                    if (!FUSE_SIM3) {
                        /* ex = uv.x - kpx in the reference; only its square is used */
                        const float is2 = A.invSigma2[min(kpLevel, A.nlevels - 1)];
                        const float exx = __fsub_rn(u, cd.x), eyy = __fsub_rn(v, cd.y);
#if !FUSE_RIG
                        if (cd.uRight >= 0.f) {
                            const float er = __fsub_rn(ur, cd.uRight);
                            const float e2 = __fadd_rn(__fadd_rn(__fmul_rn(exx, exx), __fmul_rn(eyy, eyy)), __fmul_rn(er, er));
                            if ((double)__fmul_rn(e2, is2) > 7.8) continue;
                        } else
#endif
                        {
                            const float e2 = __fadd_rn(__fmul_rn(exx, exx), __fmul_rn(eyy, eyy));
                            if ((double)__fmul_rn(e2, is2) > 5.99) continue;
                        }
                    }
                    const uint4 ta = ((const uint4*)FUSE_KF_DESC)[(size_t)c * 2], tb = ((const uint4*)FUSE_KF_DESC)[(size_t)c * 2 + 1];
                    const uint32_t dist = si_hamming(da, db, ta, tb);
                    if (dist > 255u) { /* `dist < bestDist`: never from bestDist = 256 (:2039); from INT_MAX (:2203, :2342) it is */
                        if (FUSE_SIM3) far = min(far, ((uint32_t)cd.cell << 12) | (uint32_t)c);
                        continue;
                    }
                    best = min(best, si_key(dist, cd.cell, (uint32_t)c));
                }
            }
        }
        const uint32_t g = wave_min_u32(best);
        int32_t idx = g == 0xFFFFFFFFu ? -1 : (int32_t)si_key_index(g) + (FUSE_OFFSET);
        int32_t bd = g == 0xFFFFFFFFu ? 256 : (int32_t)si_key_dist(g);
        if (g == 0xFFFFFFFFu && FUSE_SIM3) { /* wave-uniform: nothing nearer than 256 */
            const uint32_t f = wave_min_u32(far);
            if (f != 0xFFFFFFFFu) idx = (int32_t)(f & 0xFFFu) + (FUSE_OFFSET);
        }
        if (lane == 0) {
            FUSE_BEST_IDX[q] = idx;
            FUSE_BEST_DIST[q] = bd;
        }
