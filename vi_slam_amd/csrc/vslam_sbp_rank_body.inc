/* vslam_sbp_rank_body.inc -- the body of k_sbp_rank, of k_sbp_rank_rig and of k_sbp_rank_kb8 (vslam_projection_kernels.hip),
 * included once in each with SBP_RANK_RIG 0 / 1 / 2.  Text and not a template over the mode set: behind a `template <bool>` body the compiler gave the
 * pinhole kernel 87 VGPRs where it has 74 as a kernel of its own (occupancy 5 instead of 6); as text its code is what it was.
 * Names from the kernel: JS, with SBP_RANK_RIG 1 the RigFrameDev R, with SBP_RANK_RIG 2 the vslam_kb8_camera cam. */
    extern __shared__ __align__(16) uint8_t sbsm[];
    SbpCand* cand = (SbpCand*)sbsm; /* nCur */
    const SbpJobDev& J = JS.job[blockIdx.y];
    const int M = JS.M;
    const auto [nLast, nCur] = sbp_counts(J);
    if ((int)blockIdx.x * SBP_QPB >= nLast) return; /* grid is sized for the capacity */
    const vslam_kp* __restrict__ lastKps = J.lastKps;
    const vslam_kp* __restrict__ curKps = J.curKps;
    const uint8_t* __restrict__ curDesc = J.curDesc;
    const uint8_t* __restrict__ mpDesc = J.mpDesc;
    const float* __restrict__ uRight = J.uRight;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SiBounds bnd = J.bnd; /* the frame's grid bounds mnMinX.. (frame.cpp:793-821) */
    const SiBounds wbnd = J.mode == 3 ? si_kf_bounds(bnd) : bnd; /* window origin / in-image test: a KeyFrame's are integers */
    const SiGridInv inv = si_grid_inv(bnd);
    for (int i = tid; i < nCur; i += 256) cand[i] = sbp_make_cand(curKps[i], uRight ? uRight[i] : -1.f, bnd, inv);
    __syncthreads();
    for (int q = blockIdx.x * SBP_QPB + wave; q < min(nLast, (int)(blockIdx.x + 1) * SBP_QPB); q += 4) {
        SbpProj pr = {};
#if SBP_RANK_RIG == 1
        if (J.flags[q] & 1) { /* mode 4; blockIdx.y: job 0 is the left branch, job 1 the right one */
            const SbpPoint pc = sbp_transform(J.Tcw, J.x3Dw[3 * q], J.x3Dw[3 * q + 1], J.x3Dw[3 * q + 2], J.gemmFloat);
            pr = sbp_proj_rig(JS, J, R, (int)blockIdx.y, pc, lastKps[q].octave, bnd);
        }
#elif SBP_RANK_RIG == 2
        (void)lastKps; /* neither mode reads a keypoint of the query side */
        if (J.mode == 3) { /* a survivor of k_s3k_gate: its record is made, k_s3k_compact put it here */
            pr = J.proj[q];
        } else if (J.flags[q] & 1) { /* mode 2 through KannalaBrandt8::project */
            const float X = J.x3Dw[3 * q], Y = J.x3Dw[3 * q + 1], Z = J.x3Dw[3 * q + 2];
            pr = sbp_proj_keyframe_kb8(JS, J, cam, q, sbp_transform(J.Tcw, X, Y, Z, J.gemmFloat), X, Y, Z, bnd);
        }
#else
        if (J.mode == 1) {
            pr = sbp_proj_tracked(JS, J, J.mps[q]);
        } else if (J.flags[q] & 1) {
            const float X = J.x3Dw[3 * q], Y = J.x3Dw[3 * q + 1], Z = J.x3Dw[3 * q + 2];
            const SbpPoint pc = sbp_transform(J.Tcw, X, Y, Z, J.gemmFloat);
            if (J.mode == 2) pr = sbp_proj_keyframe(JS, J, q, pc, X, Y, Z, bnd);
            else if (J.mode == 3) pr = sbp_proj_sim3(JS, J, q, pc, X, Y, Z, wbnd);
            else pr = sbp_proj_last_frame(JS, J, pc, lastKps[q].octave, bnd);
        }
#endif
        /* per-lane sorted prefix (ascending), then an M-way merge across the wave */
        uint32_t best[SI_MAX_M];
#pragma unroll
        for (int j = 0; j < SI_MAX_M; j++) best[j] = 0xFFFFFFFFu;
        if (pr.valid) { /* wave-uniform */
            const SiWindow win = si_window_b(pr.u, pr.v, pr.radius, wbnd, inv);
            if (!win.empty) {
                const uint4 da = ((const uint4*)mpDesc)[(size_t)q * 2], db = ((const uint4*)mpDesc)[(size_t)q * 2 + 1];
                for (int c = lane; c < nCur; c += 64) {
                    const SbpCand cd = cand[c];
                    if (cd.cell == 0xFFFF || !sbp_candidate_ok(cd, win, pr)) continue;
                    const uint4 ta = ((const uint4*)curDesc)[(size_t)c * 2], tb = ((const uint4*)curDesc)[(size_t)c * 2 + 1];
                    uint32_t key = si_key(si_hamming(da, db, ta, tb), cd.cell, (uint32_t)c);
#pragma unroll
                    for (int j = 0; j < SI_MAX_M; j++) { /* insertion: keeps best[] ascending, drops the largest */
                        const uint32_t lo = min(key, best[j]);
                        key = max(key, best[j]);
                        best[j] = lo;
                    }
                }
            }
        }
        uint32_t mine = 0xFFFFFFFFu;
        for (int j = 0; j < M; j++) {
            const uint32_t g = wave_min_u32(best[0]);
            if (g == 0xFFFFFFFFu) break;
            if (lane == j) mine = g;
            if (best[0] == g) { /* pop (keys are unique: they contain i2) */
#pragma unroll
                for (int t = 0; t + 1 < SI_MAX_M; t++) best[t] = best[t + 1];
                best[SI_MAX_M - 1] = 0xFFFFFFFFu;
            }
        }
        if (lane < M) J.topm[(size_t)q * M + lane] = mine;
        if (lane == 0) J.proj[q] = pr;
    }
