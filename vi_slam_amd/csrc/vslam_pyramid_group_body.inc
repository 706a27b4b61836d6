/* Body of k_pyramid_group / k_pyramid_group_fit (vslam_image_kernels.hip includes it once per kernel with PYR_FIT = 0 / 1): the
 * kernels differ in the launch bound and in when the quad records are fetched, and the resident plans' kernel has to compile
 * exactly as it did before the ping-pong plans existed -- through a shared inline function its argument loads and schedule
 * came out differently (1080p pyramid alone 144 -> 151 us).  Uses the kernel's parameters and NT by name. */
    extern __shared__ __align__(16) uint8_t psm[];
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); /* wave-uniform, and said so: the row loops go scalar */
    /* the pass's first launch also zeroes the (total, overflow) header of every slot's candidate buffer and the
     * quadtree's error word (FAST and the quadtree come later on the stream): no launch of its own for 33 stores */
    if (reset_cand && blockIdx.x == 0) {
        if ((int)threadIdx.x < nslots) *(uint2*)(reset_cand + (size_t)threadIdx.x * cand_stride) = make_uint2(0u, 0u);
        if (reset_err && threadIdx.x < 4) reset_err[threadIdx.x] = 0;
    }
    /* XCD-aware order: the (slot, tile) list is cut into 8 contiguous parts, one per XCD (workgroups b, b+8 share an L2),
     * so the tiles of one image -- whose source halos overlap -- are fetched through one L2 */
    const int nwork = G.ntiles * nslots, per_xcd = (nwork + 7) >> 3;
    const int wk = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (wk >= nwork) return;
    const int slot = wk / G.ntiles, tile = wk - slot * G.ntiles;
    const PyrTileDev* T = G.tiles + (size_t)tile * (G.nl + 1);
    const PyrTileDev S0 = T[0];
    if (S0.nr <= 0 || S0.nc <= 0) return; /* a tile that owns nothing (more tiles than quads on a tiny level) */

    /* Everything a level needs besides pixels is fetched NOW, so that no global-memory latency sits inside the per-level
     * loops: the lane's quad record of every level (registers; PYR_FIT: of the first level, the others one level ahead) and
     * the row tables of every level (LDS). */
    uint4 qsel[VSLAM_PYR_GROUP_LEVELS], qcf[VSLAM_PYR_GROUP_LEVELS];
    int qloc[VSLAM_PYR_GROUP_LEVELS];
#define PYR_QUAD_RECORD(J)                                                      \
    {                                                                           \
        qsel[(J) - 1] = qcf[(J) - 1] = make_uint4(0, 0, 0, 0);                  \
        qloc[(J) - 1] = 0;                                                      \
        if ((J) <= G.nl && lane < (T[J].nc >> 2)) {                             \
            const int q_ = (T[J].c0 >> 2) + lane;                               \
            qloc[(J) - 1] = (int)G.qbase[(J) - 1][q_] - T[(J) - 1].c0;          \
            qsel[(J) - 1] = *(const uint4*)G.quads[(J) - 1][q_].sel;            \
            qcf[(J) - 1] = *(const uint4*)G.quads[(J) - 1][q_].coef;            \
        }                                                                       \
    }
#pragma unroll
    for (int j = 1; j <= VSLAM_PYR_GROUP_LEVELS; j++) {
        if constexpr (!PYR_FIT) {
            qsel[j - 1] = qcf[j - 1] = make_uint4(0, 0, 0, 0);
            qloc[j - 1] = 0;
            if (j <= G.nl) {
                const PyrTileDev D = T[j];
                if (lane < (D.nc >> 2)) {
                    const int q = (D.c0 >> 2) + lane;
                    qloc[j - 1] = (int)G.qbase[j - 1][q] - T[j - 1].c0;
                    qsel[j - 1] = *(const uint4*)G.quads[j - 1][q].sel;
                    qcf[j - 1] = *(const uint4*)G.quads[j - 1][q].coef;
                }
                uint2* rt = (uint2*)(psm + D.rt_off);
                for (int i = threadIdx.x; i < D.nr; i += NT) {
                    const int r = D.r0 + i;
                    rt[i] = make_uint2(*(const uint32_t*)(G.ytab[j - 1] + 2 * r), *(const uint32_t*)(G.yb[j - 1] + 2 * r));
                }
            }
        } else {
            if (j == 1) PYR_QUAD_RECORD(j)
            if (j <= G.nl) {
                const PyrTileDev D = T[j];
                uint2* rt = (uint2*)(psm + D.rt_off);
                for (int i = threadIdx.x; i < D.nr; i += NT) {
                    const int r = D.r0 + i;
                    rt[i] = make_uint2(*(const uint32_t*)(G.ytab[j - 1] + 2 * r), *(const uint32_t*)(G.yb[j - 1] + 2 * r));
                }
            }
        }
    }
    {   /* stage the source tile: lane = one 16-byte chunk of a row, several rows per wave instruction; the loads of
         * four such instructions are issued before the first LDS store */
        int spitch;
        const uint8_t* img = level_base_v2(pyr, slot_stride, src, G.lg[0], G.l0, slot, &spitch);
        /* bytes of a row that may be read: internal levels are padded to their pitch; of the caller's level-0 image
         * only the LAST row ends with the buffer (reading a few bytes into the next row is harmless) */
        const int readable = G.l0 == 0 ? G.readable_w0 : spitch;
        const int last_row = G.lg[0].h - 1;
        const uint32_t s0pitch = (uint32_t)__builtin_amdgcn_readfirstlane((int)S0.pitch);
        const int nch = (int)s0pitch >> 4, rpi = 64 / nch;
        const int rsub = lane / nch, ch = lane - rsub * nch;
        const bool lact = rsub < rpi;
        const int col = S0.c0 + 16 * ch;
        for (int kb = 0; kb * NW * rpi < S0.nr; kb += 4) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int row = ((kb + u) * NW + wave) * rpi + rsub;
                v[u] = make_uint4(0, 0, 0, 0);
                if (lact && row < S0.nr) {
                    const uint8_t* gp = img + mad24u_s((uint32_t)(S0.r0 + row), (uint32_t)spitch, (uint32_t)col); /* 32-bit, full rate */
                    if (col + 16 <= readable || (G.l0 == 0 && S0.r0 + row < last_row)) v[u] = *(const uint4*)gp;
                    else if (col < readable) v[u] = pyr_load16_tail(gp, readable - col);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int row = ((kb + u) * NW + wave) * rpi + rsub;
                if (lact && row < S0.nr) *(uint4*)(psm + mad24u_s((uint32_t)row, s0pitch, S0.lds_off + 16u * (uint32_t)ch)) = v[u];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 1; j <= VSLAM_PYR_GROUP_LEVELS; j++) {
        if (j > G.nl) break; /* uniform */
        if (PYR_FIT && j < VSLAM_PYR_GROUP_LEVELS) PYR_QUAD_RECORD(j + 1) /* in flight while this level is computed */
        /* the tile records are the same for every lane -- said so field by field (16-bit fields come through vector loads):
         * row addresses are then scalar multiplies instead of vector ones in the row loop */
        const PyrTileU S = pyr_tile_uniform(T[j - 1]), D = pyr_tile_uniform(T[j]);
        if (lane < (D.nc >> 2) && D.nr > 0) {
            const int q = (D.c0 >> 2) + lane;
            const int loc = qloc[j - 1];
            const uint32_t sh = (uint32_t)(loc & 3);
            const uint4 sel = qsel[j - 1], cf = qcf[j - 1];
            const int sp = (int)S.pitch, dp = (int)D.pitch;
            const int sbase = (int)S.lds_off + (loc & ~3) - __mul24((int)S.r0, sp); /* + source row * sp */
            const int dbase = (int)D.lds_off + 4 * lane - __mul24((int)D.r0, dp);   /* + row * dp */
            const bool qstore = q >= D.sq0 && q < D.sq1;
            uint8_t* gout = pyr + (size_t)slot * slot_stride + G.lg[j].off + 4 * (size_t)q;
            const int gpitch = G.lg[j].pitch;
            const uint2* rt = (const uint2*)(psm + D.rt_off) - D.r0; /* indexed by the absolute row */
            /* A wave owns a contiguous band of output rows and walks it top to bottom.  Consecutive output rows share a
             * source row (sy1 of row r is sy0 of row r + 1 for 5 rows out of 6 at scale 1.2), so the horizontal pass
             * of a source row -- (h >> 4) of the lane's four pixels -- is kept in registers and reused: 1.2 instead of
             * 2 horizontal passes per output row. */
            const int band = (D.nr + NW - 1) / NW;
            const int rb = D.r0 + wave * band, re = min(rb + band, D.r0 + D.nr);
            int prev_sy = -1;
            int hp0 = 0, hp1 = 0, hp2 = 0, hp3 = 0;
#define PYR_HPASS(SY, H0, H1, H2, H3)                                                                        \
    {                                                                                                         \
        const uint32_t* pr_ = (const uint32_t*)(psm + sbase + __mul24((int)(SY), sp));                        \
        const uint32_t x0_ = pr_[0], x1_ = pr_[1], x2_ = pr_[2];                                             \
        const uint32_t lo_ = __builtin_amdgcn_alignbyte(x1_, x0_, sh), hi_ = __builtin_amdgcn_alignbyte(x2_, x1_, sh); \
        hdot2x4(__builtin_amdgcn_perm(hi_, lo_, sel.x), __builtin_amdgcn_perm(hi_, lo_, sel.y),                \
                __builtin_amdgcn_perm(hi_, lo_, sel.z), __builtin_amdgcn_perm(hi_, lo_, sel.w), cf, &H0, &H1, &H2, &H3); \
        H0 >>= 4; H1 >>= 4; H2 >>= 4; H3 >>= 4;                                                               \
    }
            for (int r = rb; r < re; r++) {
                const uint2 e = rt[r];
                /* wave-uniform by construction (LDS broadcast of the row table): scalar branches */
                const int sy0 = __builtin_amdgcn_readfirstlane((int)(e.x & 0xFFFF));
                const int sy1 = __builtin_amdgcn_readfirstlane((int)(e.x >> 16));
                const int b0 = (int)(int16_t)(e.y & 0xFFFF), b1 = (int)e.y >> 16; /* 0 .. 2048 */
                int g0, g1, g2, g3;
                if (sy0 == prev_sy) {
                    g0 = hp0; g1 = hp1; g2 = hp2; g3 = hp3;
                } else
                    PYR_HPASS(sy0, g0, g1, g2, g3)
                if (sy1 != sy0) PYR_HPASS(sy1, hp0, hp1, hp2, hp3)
                else {
                    hp0 = g0; hp1 = g1; hp2 = g2; hp3 = g3;
                }
                prev_sy = sy1;
                /* vertical pass: both factors fit 24 bits (b <= 2048, h >> 4 <= 32640): full-rate v_mul_i32_i24 */
                const uint32_t v0 = (uint32_t)(((__mul24(b0, g0) >> 16) + (__mul24(b1, hp0) >> 16) + 2) >> 2);
                const uint32_t v1 = (uint32_t)(((__mul24(b0, g1) >> 16) + (__mul24(b1, hp1) >> 16) + 2) >> 2);
                const uint32_t v2 = (uint32_t)(((__mul24(b0, g2) >> 16) + (__mul24(b1, hp2) >> 16) + 2) >> 2);
                const uint32_t v3 = (uint32_t)(((__mul24(b0, g3) >> 16) + (__mul24(b1, hp3) >> 16) + 2) >> 2);
                const uint32_t out = (v0 & 0xFF) | ((v1 & 0xFF) << 8) | ((v2 & 0xFF) << 16) | (v3 << 24);
                *(uint32_t*)(psm + dbase + __mul24(r, dp)) = out;
                if (qstore && r >= D.sr0 && r < D.sr1) *(uint32_t*)(gout + (size_t)r * gpitch) = out;
            }
#undef PYR_HPASS
        }
        __syncthreads();
    }
#undef PYR_QUAD_RECORD
