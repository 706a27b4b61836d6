/* vslam_host.cpp -- see vslam_host.h.  Reference lines are cited per function. */
#include "vslam_host.h"
#include "vslam_undistort.h"
#include "vslam_frustum.h"
#include "vslam_kb8.h"
#include "vslam_two_view.h"
#include "vslam_matchdev.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace vslam {

/* cvRound / cvFloor / cvCeil as OpenCV 4.2 defines them on x86-64 (fast_math.hpp): SSE round-to-nearest-even */
static inline int cv_round(float v) { return (int)lrintf(v); }
static inline int cv_round(double v) { return (int)lrint(v); }
static inline int cv_floor(float v) {
    int i = (int)v;
    return i - (i > v);
}
static inline int cv_ceil(float v) {
    int i = (int)v;
    return i + (i < v);
}
static inline int16_t sat_short(float v) {
    int iv = cv_round(v);
    return (int16_t)std::min(std::max(iv, (int)SHRT_MIN), (int)SHRT_MAX);
}

void build_tables(int nfeatures, float scaleFactorF, int nlevels, ExtractorTables& t) {
    /* fextractor.cpp:401-461; scaleFactor is a double member initialised from the float argument */
    const double scaleFactor = scaleFactorF;
    t.nlevels = nlevels;
    t.scale.assign(nlevels, 1.0f);
    t.sigma2.assign(nlevels, 1.0f);
    for (int i = 1; i < nlevels; i++) {
        t.scale[i] = (float)(t.scale[i - 1] * scaleFactor);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    t.inv_scale.resize(nlevels);
    t.inv_sigma2.resize(nlevels);
    for (int i = 0; i < nlevels; i++) {
        t.inv_scale[i] = 1.0f / t.scale[i];
        t.inv_sigma2[i] = 1.0f / t.sigma2[i];
    }
    t.quota.assign(nlevels, 0);
    const float factor = (float)(1.0f / scaleFactor);
    float want = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int level = 0; level < nlevels - 1; level++) {
        t.quota[level] = cv_round(want);
        sum += t.quota[level];
        want *= factor;
    }
    t.quota[nlevels - 1] = std::max(nfeatures - sum, 0);

    /* umax (fextractor.cpp:445-460) */
    const int HP = 15;
    int v, v0;
    const int vmax = cv_floor(HP * sqrtf(2.f) / 2 + 1);
    const int vmin = cv_ceil(HP * sqrtf(2.f) / 2);
    const double hp2 = HP * HP;
    for (v = 0; v <= vmax; ++v) t.umax[v] = cv_round(sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    t.disc_u.clear();
    t.disc_v.clear();
    for (v = -HP; v <= HP; v++) {
        const int d = t.umax[std::abs(v)];
        for (int u = -d; u <= d; u++) {
            t.disc_u.push_back((int8_t)u);
            t.disc_v.push_back((int8_t)v);
        }
    }
}

void level_size(const ExtractorTables& t, int w, int h, int level, int* lw, int* lh) {
    const float scale = t.inv_scale[level];
    *lw = cv_round((float)w * scale);
    *lh = cv_round((float)h * scale);
}

void build_resize_tables(int sw, int sh, int dw, int dh, ResizeTables& r) {
    /* OpenCV 4.2 resize.cpp, INTER_LINEAR, depth 8U: coefficients in 11-bit fixed point */
    const int ONE = 2048;
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    r.xtab.resize(2 * dw);
    r.xa.resize(2 * dw);
    r.ytab.resize(2 * dh);
    r.yb.resize(2 * dh);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; } /* dx >= xmax: D = S[sx] * ONE */
        r.xtab[2 * dx] = (uint16_t)sx;
        r.xtab[2 * dx + 1] = (uint16_t)std::min(sx + 1, sw - 1);
        r.xa[2 * dx] = sat_short((1.f - fx) * ONE);
        r.xa[2 * dx + 1] = sat_short(fx * ONE);
    }
    auto clip = [](int x, int a, int b) { return x >= a ? (x < b ? x : b - 1) : a; };
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        r.ytab[2 * dy] = (uint16_t)clip(sy, 0, sh);
        r.ytab[2 * dy + 1] = (uint16_t)clip(sy + 1, 0, sh);
        r.yb[2 * dy] = sat_short((1.f - fy) * ONE);
        r.yb[2 * dy + 1] = sat_short(fy * ONE);
    }
}

bool build_resize_quads(const ResizeTables& r, int sw, int dw, std::vector<uint16_t>& qbase,
                        std::vector<uint32_t>& quads) {
    if (sw < 8) return false;
    const int nq = (dw + 3) / 4;
    qbase.assign(nq, 0);
    quads.assign((size_t)nq * 8, 0);
    for (int q = 0; q < nq; q++) {
        int lo = 1 << 30, hi = -1;
        for (int j = 0; j < 4; j++) {
            const int dx = std::min(4 * q + j, dw - 1); /* outputs past the row end repeat the last column */
            lo = std::min(lo, (int)r.xtab[2 * dx]);
            hi = std::max(hi, (int)r.xtab[2 * dx + 1]);
        }
        const int base = std::min(lo, sw - 8); /* the 8-byte window must stay inside the source row */
        if (hi - base > 7) return false;
        qbase[q] = (uint16_t)base;
        for (int j = 0; j < 4; j++) {
            const int dx = std::min(4 * q + j, dw - 1);
            const uint32_t o0 = r.xtab[2 * dx] - base, o1 = r.xtab[2 * dx + 1] - base;
            quads[(size_t)q * 8 + j] = o0 | (0x0cu << 8) | (o1 << 16) | (0x0cu << 24);
            quads[(size_t)q * 8 + 4 + j] = (uint32_t)(uint16_t)r.xa[2 * dx] | ((uint32_t)(uint16_t)r.xa[2 * dx + 1] << 16);
        }
    }
    return true;
}


/* ------------------------------------------------------------------ fused pyramid plan (k_pyramid_group) */
static inline int div_floor4(int x) { return x >> 2; }

static bool plan_with(const std::vector<const PyrLevelTables*>& tabs, int l0, int ntx, int nty, size_t max_lds,
                      bool pingpong, PyrGroupPlan& plan) {
    const int nl = (int)tabs.size();
    plan.l0 = l0;
    plan.nl = nl;
    plan.ntx = ntx;
    plan.nty = nty;
    plan.tiles.assign((size_t)ntx * nty * (nl + 1), PyrTileLevel{});
    size_t lds_max = 0;
    for (int ty = 0; ty < nty; ty++)
        for (int tx = 0; tx < ntx; tx++) {
            PyrTileLevel* T = &plan.tiles[((size_t)ty * ntx + tx) * (nl + 1)];
            /* compute ranges, deepest level first: C_j = hull(own_j, need of level j+1) */
            int cq0[VSLAM_MAX_LEVELS + 1], cq1[VSLAM_MAX_LEVELS + 1], cr0[VSLAM_MAX_LEVELS + 1], cr1[VSLAM_MAX_LEVELS + 1];
            int nq0 = -1, nq1 = -1, nr0 = -1, nr1 = -1; /* need on the current level from the deeper one (empty: -1) */
            for (int j = nl; j >= 0; j--) {
                int oq0 = 0, oq1 = 0, or0 = 0, or1 = 0;
                if (j >= 1) {
                    const PyrLevelTables& t = *tabs[j - 1];
                    const int nq = (t.dw + 3) / 4;
                    oq0 = (int)((long long)tx * nq / ntx);
                    oq1 = (int)((long long)(tx + 1) * nq / ntx);
                    or0 = (int)((long long)ty * t.dh / nty);
                    or1 = (int)((long long)(ty + 1) * t.dh / nty);
                    T[j].sq0 = (int16_t)oq0; T[j].sq1 = (int16_t)oq1; T[j].sr0 = (int16_t)or0; T[j].sr1 = (int16_t)or1;
                }
                const bool own = j >= 1 && oq1 > oq0 && or1 > or0, need = nq1 > nq0 && nr1 > nr0;
                if (!own && !need) { cq0[j] = cq1[j] = cr0[j] = cr1[j] = 0; }
                else if (own && need) {
                    cq0[j] = std::min(oq0, nq0); cq1[j] = std::max(oq1, nq1);
                    cr0[j] = std::min(or0, nr0); cr1[j] = std::max(or1, nr1);
                } else if (own) { cq0[j] = oq0; cq1[j] = oq1; cr0[j] = or0; cr1[j] = or1; }
                else { cq0[j] = nq0; cq1[j] = nq1; cr0[j] = nr0; cr1[j] = nr1; }
                nq0 = nq1 = nr0 = nr1 = -1;
                if (j >= 1 && cq1[j] > cq0[j]) { /* what computing C_j reads of level j-1 */
                    const PyrLevelTables& t = *tabs[j - 1];
                    const int dxl = std::min(4 * cq1[j], t.dw) - 1;
                    const int lo = t.qbase[cq0[j]];               /* windows start here (<= the first tap) */
                    const int hi = t.r.xtab[2 * dxl + 1];          /* last tap column */
                    nq0 = div_floor4(lo);
                    nq1 = div_floor4(hi) + 1;
                    nr0 = t.r.ytab[2 * cr0[j]];
                    nr1 = t.r.ytab[2 * (cr1[j] - 1) + 1] + 1;
                }
            }
            /* LDS layout.  Every level resident: the tiles follow each other.  Ping-pong: level j reads only level j-1, and
             * the barrier after level j-1 ends the last read of level j-2, so two regions are enough -- the even entries
             * (source, level 2, ...) share region 0, the odd ones region 1, each as large as its largest tenant. */
            size_t region[2] = {0, 0};
            for (int j = 0; j <= nl; j++) {
                T[j].c0 = (int16_t)(4 * cq0[j]);
                T[j].nc = (int16_t)(4 * (cq1[j] - cq0[j]));
                T[j].r0 = (int16_t)cr0[j];
                T[j].nr = (int16_t)(cr1[j] - cr0[j]);
                T[j].pitch = (uint32_t)((T[j].nc + 8 + 15) & ~15);
                region[j & 1] = std::max(region[j & 1], (size_t)T[j].pitch * T[j].nr);
                if (j >= 1 && T[j].nc / 4 > 64) return false; /* lane = quad */
                if (j == 0 && T[j].pitch / 16 > 64) return false; /* staging: lane = 16-byte chunk of a row */
            }
            size_t off = 0;
            for (int j = 0; j <= nl; j++) {
                if (pingpong) T[j].lds_off = (uint32_t)((j & 1) ? region[0] : 0);
                else {
                    T[j].lds_off = (uint32_t)off;
                    off += (size_t)T[j].pitch * T[j].nr;
                }
            }
            if (pingpong) {
                off = region[0] + region[1];
                /* what level j overwrites must be dead: its tile may not touch the level it is computed from (each region
                 * is as large as its largest tenant, so a tile cannot leave its region) */
                for (int j = 1; j <= nl; j++) {
                    const size_t d0 = T[j].lds_off, d1 = d0 + (size_t)T[j].pitch * T[j].nr;
                    const size_t s0 = T[j - 1].lds_off, s1 = s0 + (size_t)T[j - 1].pitch * T[j - 1].nr;
                    if (d0 < s1 && s0 < d1) return false;
                }
            }
            for (int j = 1; j <= nl; j++) {
                T[j].rt_off = (uint32_t)off;
                off += ((size_t)T[j].nr * 8 + 15) & ~(size_t)15;
            }
            lds_max = std::max(lds_max, off + 16);
        }
    plan.lds_bytes = lds_max;
    return lds_max <= max_lds;
}

void pyramid_tile_shape(int width, int height, int batch, int tune_rows, int tune_pingpong, int* rows, bool* pingpong,
                        size_t* max_lds) {
    /* contexts of one or two images keep every level resident: their 16-row tiles are small anyway and nothing runs beside
     * them; so do frames above a megapixel, whose step lost 4 % with the ping-pong tiles (KITTI mono +4 %, 32 rows the best
     * of 24 / 28 / 32 / 36 / 40: profiles/pyramid_beside_fast_ab.txt).  vslam_fe_create plans the resident shape as well for
     * the passes of the stereo-frame entry */
    *pingpong = tune_pingpong >= 0 ? tune_pingpong != 0 : batch > 2 && (size_t)width * height <= 1000000;
    *rows = tune_rows >= 0 ? tune_rows
            : batch <= 2 ? 16 : *pingpong ? 32 : (size_t)width * height > 1000000 ? 40 : 48;
    *max_lds = *pingpong ? (size_t)VSLAM_PYR_PINGPONG_LDS : (size_t)VSLAM_PYR_LDS_KB * 1024;
}

bool build_pyramid_group(const std::vector<const PyrLevelTables*>& tabs, int l0, size_t max_lds, PyrGroupPlan& plan, int rows_override,
                         bool pingpong) {
    if (tabs.empty() || tabs.size() > VSLAM_MAX_LEVELS) return false;
    for (const PyrLevelTables* t : tabs)
        if (!t || t->qbase.empty()) return false; /* a level without the quad table: per-level launches */
    const int nq1 = (tabs[0]->dw + 3) / 4, h1 = tabs[0]->dh;
    /* output rows of the first computed level per tile (vslam_tuning.pyr_rows for A/B runs).  Taller tiles recompute less
     * halo and amortise the per-tile prologue over more rows: 28 -> 48 rows is +3 % mono, +2 % stereo, +3 % at 1080p in the
     * pipeline (36 / 40 / 48 / 56 / 64 measured; the LDS limit of the plan, 64 KB, is the brake at 64) */
    int rows = 48;
    if (rows_override >= 0) rows = std::min(64, std::max(4, rows_override));
    const int nty = std::max(1, (h1 + rows - 1) / rows);
#ifndef VSLAM_PYR_TILE_QUADS
#define VSLAM_PYR_TILE_QUADS 52 /* widest tile tried first: quads of the first computed level (a wave's lanes, halo included) */
#endif
    for (int ntx = std::max(1, (nq1 + VSLAM_PYR_TILE_QUADS - 1) / VSLAM_PYR_TILE_QUADS); ntx <= std::max(1, nq1 / 8); ntx++)
        if (plan_with(tabs, l0, ntx, nty, max_lds, pingpong, plan)) return true;
    return false;
}

int emulate_pyramid_group(const PyrGroupPlan& plan, const std::vector<const PyrLevelTables*>& tabs,
                          const uint8_t* src, int sstride, int readable_w, std::vector<uint8_t*>& dst,
                          const std::vector<int>& dstride) {
    const int nl = plan.nl;
    std::vector<uint8_t> lds(plan.lds_bytes), ok(plan.lds_bytes);
    for (int tile = 0; tile < plan.ntx * plan.nty; tile++) {
        const PyrTileLevel* T = &plan.tiles[(size_t)tile * (nl + 1)];
        std::fill(lds.begin(), lds.end(), (uint8_t)0xCD);
        std::fill(ok.begin(), ok.end(), (uint8_t)0);
        if (T[0].nr <= 0 || T[0].nc <= 0) continue;
        /* stage the source tile: dwords of columns [c0, c0 + pitch), those inside the readable row width */
        for (int r = 0; r < T[0].nr; r++)
            for (int c = 0; c < (int)T[0].pitch; c++) {
                const int col = T[0].c0 + c;
                const size_t a = T[0].lds_off + (size_t)r * T[0].pitch + c;
                if (a >= lds.size()) return -1;
                if (col < readable_w) {
                    lds[a] = src[(size_t)(T[0].r0 + r) * sstride + col];
                    ok[a] = 1;
                }
            }
        for (int j = 1; j <= nl; j++) {
            const PyrLevelTables& t = *tabs[j - 1];
            const PyrTileLevel &S = T[j - 1], &D = T[j];
            {   /* the level's tile may lie over an earlier level's (ping-pong layout): not over the one it reads, not over
                 * a row table, and what the earlier tenant left there does not count as computed */
                const size_t d0 = D.lds_off, d1 = d0 + (size_t)D.pitch * D.nr;
                const size_t s0 = S.lds_off, s1 = s0 + (size_t)S.pitch * S.nr;
                if (d1 > lds.size()) return -7;
                if (d0 < s1 && s0 < d1) return -8;
                for (int k = 1; k <= nl; k++)
                    if (T[k].nr > 0 && d1 > T[k].rt_off) return -9;
                std::fill(ok.begin() + d0, ok.begin() + d1, (uint8_t)0);
                std::fill(lds.begin() + d0, lds.begin() + d1, (uint8_t)0xCD);
            }
            for (int r = D.r0; r < D.r0 + D.nr; r++) {
                const int sy0 = t.r.ytab[2 * r], sy1 = t.r.ytab[2 * r + 1], b0 = t.r.yb[2 * r], b1 = t.r.yb[2 * r + 1];
                if (sy0 < S.r0 || sy1 >= S.r0 + S.nr) return -2;
                for (int lane = 0; lane < D.nc / 4; lane++) {
                    const int q = D.c0 / 4 + lane;
                    const int loc = (int)t.qbase[q] - S.c0;
                    if (loc < 0) return -3;
                    const int dwb = loc & ~3, sh = loc & 3;
                    if (dwb + 12 > (int)S.pitch) return -4;
                    uint32_t out = 0;
                    for (int k = 0; k < 4; k++) {
                        const uint32_t sel = t.quads[(size_t)q * 8 + k], cf = t.quads[(size_t)q * 8 + 4 + k];
                        const int o0 = sel & 0xFF, o1 = (sel >> 16) & 0xFF;
                        const int a0 = (int16_t)(cf & 0xFFFF), a1 = (int16_t)(cf >> 16);
                        int h[2];
                        for (int rr = 0; rr < 2; rr++) {
                            const size_t base = S.lds_off + (size_t)((rr ? sy1 : sy0) - S.r0) * S.pitch + dwb + sh;
                            if (base + 8 > lds.size()) return -5;
                            if (!ok[base + o0] || !ok[base + o1]) return -6; /* a tap that was never staged/computed */
                            h[rr] = lds[base + o0] * a0 + lds[base + o1] * a1;
                        }
                        const int v = (((b0 * (h[0] >> 4)) >> 16) + ((b1 * (h[1] >> 4)) >> 16) + 2) >> 2;
                        out |= (uint32_t)(v & 0xFF) << (8 * k);
                    }
                    const size_t da = D.lds_off + (size_t)(r - D.r0) * D.pitch + 4 * lane;
                    if (da + 4 > lds.size()) return -7;
                    for (int k = 0; k < 4; k++) {
                        lds[da + k] = (uint8_t)(out >> (8 * k));
                        ok[da + k] = 1;
                    }
                    if (q >= D.sq0 && q < D.sq1 && r >= D.sr0 && r < D.sr1)
                        for (int k = 0; k < 4; k++)
                            if (4 * q + k < dstride[j]) dst[j][(size_t)r * dstride[j] + 4 * q + k] = (uint8_t)(out >> (8 * k));
                }
            }
        }
    }
    return 0;
}

void build_cells(int level, int lw, int lh, std::vector<HostCell>& out) {
    /* fextractor.cpp:764-797 */
    const float W = 30;
    const int minBorderX = VSLAM_FAST_BORDER, minBorderY = VSLAM_FAST_BORDER;
    const int maxBorderX = lw - VSLAM_FAST_BORDER, maxBorderY = lh - VSLAM_FAST_BORDER;
    const float width = (float)(maxBorderX - minBorderX);
    const float height = (float)(maxBorderY - minBorderY);
    const int nCols = (int)(width / W);
    const int nRows = (int)(height / W);
    if (nCols < 1 || nRows < 1) return;
    const int wCell = (int)std::ceil(width / nCols);
    const int hCell = (int)std::ceil(height / nRows);
    for (int i = 0; i < nRows; i++) {
        const float iniY = (float)(minBorderY + i * hCell);
        float maxY = iniY + hCell + 6;
        if (iniY >= maxBorderY - 3) continue;
        if (maxY > maxBorderY) maxY = (float)maxBorderY;
        for (int j = 0; j < nCols; j++) {
            const float iniX = (float)(minBorderX + j * wCell);
            float maxX = iniX + wCell + 6;
            if (iniX >= maxBorderX - 6) continue;
            if (maxX > maxBorderX) maxX = (float)maxBorderX;
            HostCell c;
            c.level = (uint16_t)level;
            c.x0 = (uint16_t)iniX;
            c.y0 = (uint16_t)iniY;
            c.x1 = (uint16_t)maxX;
            c.y1 = (uint16_t)maxY;
            if (c.x1 - c.x0 < 7 || c.y1 - c.y0 < 7) continue; /* cv::FAST finds nothing in < 7 px */
            out.push_back(c);
        }
    }
}

void build_bands(const std::vector<HostCell>& cells, int max_cells, int max_width, std::vector<HostBand>& out) {
    const size_t n = cells.size();
    size_t i = 0;
    while (i < n) {
        /* the cells of one cell row: same level, same window rows */
        size_t e = i + 1;
        while (e < n && cells[e].level == cells[i].level && cells[e].y0 == cells[i].y0 && cells[e].y1 == cells[i].y1 &&
               cells[e].x0 > cells[e - 1].x0)
            e++;
        const int nrow = (int)(e - i);
        /* pitch of the cells in x; a row of one cell is its own pitch */
        const int wcell = nrow > 1 ? cells[i + 1].x0 - cells[i].x0 : std::max(1, cells[i].x1 - cells[i].x0 - 6);
        const int per = std::max(1, std::min(max_cells, max_width / std::max(wcell, 1)));
        for (size_t b = i; b < e; b += (size_t)per) {
            const size_t last = std::min(e, b + (size_t)per) - 1;
            HostBand hb;
            hb.cell0 = (uint32_t)b;
            hb.level = cells[b].level;
            hb.ncell = (uint16_t)(last - b + 1);
            hb.wcell = (uint16_t)wcell;
            hb.x0 = cells[b].x0;
            hb.y0 = cells[b].y0;
            hb.ww = (uint16_t)(cells[last].x1 - cells[b].x0);
            hb.wh = (uint16_t)(cells[b].y1 - cells[b].y0);
            out.push_back(hb);
        }
        i = e;
    }
}

/* ------------------------------------------------------------------ quadtree distribution */
namespace {
struct QNode {
    int x0, y0, x1, y1; /* UL.x, UL.y, UR.x(=BR.x), BR.y(=BL.y) */
    int begin, count;   /* range in the permutation array (vKeys, order preserved) */
    int prev, next;     /* std::list links */
    bool noMore;
};

struct QTree {
    std::vector<QNode> pool; /* index == creation order (the tie-break key) */
    std::vector<int> perm, tmp;
    const Cand* c;
    int head = -1, tail = -1, size = 0;

    int push_front(const QNode& n) {
        int id = (int)pool.size();
        pool.push_back(n);
        pool[id].prev = -1;
        pool[id].next = head;
        if (head >= 0) pool[head].prev = id;
        head = id;
        if (tail < 0) tail = id;
        size++;
        return id;
    }
    int push_back(const QNode& n) {
        int id = (int)pool.size();
        pool.push_back(n);
        pool[id].next = -1;
        pool[id].prev = tail;
        if (tail >= 0) pool[tail].next = id;
        tail = id;
        if (head < 0) head = id;
        size++;
        return id;
    }
    void erase(int id) {
        const int p = pool[id].prev, nx = pool[id].next;
        if (p >= 0) pool[p].next = nx; else head = nx;
        if (nx >= 0) pool[nx].prev = p; else tail = p;
        size--;
    }
    /* ExtractorNode::DivideNode (fextractor.cpp:472-528): children in order n1..n4, each keeps the
     * parent's key order; returns child ids (or -1 if empty) after push_front in that order. */
    void divide(int id, int child[4]) {
        const QNode P = pool[id];
        const int halfX = (P.x1 - P.x0 + 1) >> 1; /* ceil((float)d/2), d >= 0 */
        const int halfY = (P.y1 - P.y0 + 1) >> 1;
        const int mx = P.x0 + halfX, my = P.y0 + halfY;
        int cnt[4] = {0, 0, 0, 0};
        for (int i = P.begin; i < P.begin + P.count; i++) {
            const Cand& k = c[perm[i]];
            const int q = (k.x < mx) ? ((k.y < my) ? 0 : 2) : ((k.y < my) ? 1 : 3);
            cnt[q]++;
        }
        int off[4] = {P.begin, P.begin + cnt[0], P.begin + cnt[0] + cnt[1], P.begin + cnt[0] + cnt[1] + cnt[2]};
        int w[4] = {off[0], off[1], off[2], off[3]};
        for (int i = P.begin; i < P.begin + P.count; i++) {
            const Cand& k = c[perm[i]];
            const int q = (k.x < mx) ? ((k.y < my) ? 0 : 2) : ((k.y < my) ? 1 : 3);
            tmp[w[q]++] = perm[i];
        }
        memcpy(&perm[P.begin], &tmp[P.begin], sizeof(int) * P.count);
        const int bx[4][4] = {{P.x0, P.y0, mx, my}, {mx, P.y0, P.x1, my}, {P.x0, my, mx, P.y1}, {mx, my, P.x1, P.y1}};
        for (int q = 0; q < 4; q++) {
            child[q] = -1;
            if (cnt[q] == 0) continue;
            QNode n;
            n.x0 = bx[q][0]; n.y0 = bx[q][1]; n.x1 = bx[q][2]; n.y1 = bx[q][3];
            n.begin = off[q];
            n.count = cnt[q];
            n.noMore = cnt[q] == 1;
            n.prev = n.next = -1;
            child[q] = push_front(n);
        }
    }
};
} // namespace

bool distribute_octree(const Cand* cands, int n, int W, int H, int N, std::vector<Cand>& out) {
    out.clear();
    const int nIni = (int)std::round((float)W / (float)H);
    if (nIni < 1) return false;
    if (n == 0) return true;
    const float hX = (float)W / nIni;
    QTree T;
    T.c = cands;
    T.perm.resize(n);
    T.tmp.resize(n);
    T.pool.reserve(4 * (size_t)std::max(N, 16) + 64);

    /* initial nodes and stable bucketing of the candidates (fextractor.cpp:543-561) */
    std::vector<int> bucket(n), cnt(nIni + 1, 0);
    for (int i = 0; i < n; i++) {
        int b = (int)((float)cands[i].x / hX);
        if (b >= nIni) b = nIni - 1;
        bucket[i] = b;
        cnt[b + 1]++;
    }
    for (int b = 0; b < nIni; b++) cnt[b + 1] += cnt[b];
    {
        std::vector<int> w(cnt.begin(), cnt.end() - 1);
        for (int i = 0; i < n; i++) T.perm[w[bucket[i]]++] = i;
    }
    for (int i = 0; i < nIni; i++) {
        QNode ni;
        ni.x0 = (int)(hX * (float)i);
        ni.x1 = (int)(hX * (float)(i + 1));
        ni.y0 = 0;
        ni.y1 = H;
        ni.begin = cnt[i];
        ni.count = cnt[i + 1] - cnt[i];
        ni.noMore = ni.count == 1;
        ni.prev = ni.next = -1;
        if (ni.count == 0) continue; /* erased at fextractor.cpp:572-573 */
        T.push_back(ni);
    }

    typedef std::pair<int, int> SP; /* (size, node id); id order == creation order */
    std::vector<SP> vSize, vPrev;
    bool bFinish = false;
    while (!bFinish) {
        int prevSize = T.size;
        int nToExpand = 0;
        vSize.clear();
        for (int cur = T.head; cur >= 0;) {
            const int next = T.pool[cur].next;
            if (!T.pool[cur].noMore) {
                int ch[4];
                T.divide(cur, ch);
                for (int q = 0; q < 4; q++)
                    if (ch[q] >= 0 && T.pool[ch[q]].count > 1) {
                        nToExpand++;
                        vSize.push_back(SP(T.pool[ch[q]].count, ch[q]));
                    }
                T.erase(cur);
            }
            cur = next;
        }
        if (T.size >= N || T.size == prevSize) {
            bFinish = true;
        } else if (T.size + nToExpand * 3 > N) {
            while (!bFinish) {
                prevSize = T.size;
                vPrev = vSize;
                vSize.clear();
                std::sort(vPrev.begin(), vPrev.end()); /* ascending (size, creation id) */
                for (int j = (int)vPrev.size() - 1; j >= 0; j--) {
                    int ch[4];
                    T.divide(vPrev[j].second, ch);
                    for (int q = 0; q < 4; q++)
                        if (ch[q] >= 0 && T.pool[ch[q]].count > 1) vSize.push_back(SP(T.pool[ch[q]].count, ch[q]));
                    T.erase(vPrev[j].second);
                    if (T.size >= N) break;
                }
                if (T.size >= N || T.size == prevSize) bFinish = true;
            }
        }
    }
    out.reserve(T.size);
    for (int cur = T.head; cur >= 0; cur = T.pool[cur].next) {
        const QNode& nd = T.pool[cur];
        int best = T.perm[nd.begin];
        int maxResponse = cands[best].response;
        for (int k = 1; k < nd.count; k++) {
            const int id = T.perm[nd.begin + k];
            if (cands[id].response > maxResponse) {
                best = id;
                maxResponse = cands[id].response;
            }
        }
        out.push_back(cands[best]);
    }
    return true;
}

/* ------------------------------------------------------------------ matcher host logic */
uint32_t oct_key_path(int x, int y, int W, int H, int depth) {
    const int nIni = (int)std::round((float)W / (float)H);
    const float hX = (float)W / (float)nIni;
    int b = (int)((float)x / hX); /* fextractor.cpp:557-561 */
    b = std::min(b, nIni - 1);
    int x0 = (int)(hX * (float)b), x1 = (int)(hX * (float)(b + 1)), y0 = 0, y1 = H;
    uint32_t code = 0;
    for (int d = 0; d < depth; d++) { /* DivideNode: halfX = ceil((UR.x - UL.x) / 2); kp.x < n1.UR.x, kp.y < n1.BR.y */
        const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
        const int qx = x < mx ? 0 : 1, qy = y < my ? 0 : 1;
        code = (code << 2) | (uint32_t)qx | ((uint32_t)qy << 1);
        if (qx) x0 = mx; else x1 = mx;
        if (qy) y0 = my; else y1 = my;
    }
    return ((uint32_t)b << (2 * depth)) | code;
}

void pack_bands(const std::vector<HostBand>& hb, int nlevels, BandTables& out) {
    out = BandTables();
    out.bands.resize(hb.size());
    std::vector<std::pair<int, int>> cls;
    bool ok = !hb.empty() && nlevels <= 16;
    for (size_t i = 0; i < hb.size(); i++) {
        const HostBand& b = hb[i];
        out.max_wh = std::max(out.max_wh, (int)b.wh);
        out.max_iw = std::max(out.max_iw, (int)b.ww - 6);
        out.max_cells = std::max(out.max_cells, (int)b.ncell);
        ok = ok && b.wcell < 256;
        const int iw = (int)b.ww - 6, wc = std::max(1, (int)b.wcell);
        size_t ci = 0;
        while (ci < cls.size() && cls[ci] != std::make_pair(wc, iw)) ci++;
        if (ci == cls.size()) {
            cls.push_back(std::make_pair(wc, iw));
            out.classes.resize(out.classes.size() + 272, 0);
            uint8_t* cb = out.classes.data() + ci * 272;
            for (int x = 0; x < 136 && x < iw; x++) {
                const int c = x / wc, cend = std::min((c + 1) * wc, iw) - 1;
                cb[x] = (uint8_t)(1u << std::min(c, 7));
                cb[136 + x] = (uint8_t)((x == c * wc ? 1 : 0) | (x == cend ? 2 : 0));
            }
        }
        out.bands[i].cell0 = b.cell0;
        out.bands[i].lnw = (uint32_t)b.level | ((uint32_t)b.ncell << 4) | ((uint32_t)b.wcell << 8) | ((uint32_t)ci << 16);
        out.bands[i].xy = (uint32_t)b.x0 | ((uint32_t)b.y0 << 16);
        out.bands[i].wh = (uint32_t)b.ww | ((uint32_t)b.wh << 16);
    }
    out.ok = ok && cls.size() < 65536;
}

int keypoint_capacity(const int* quota, const int* lw, const int* lh, int nlevels, int nfeatures) {
    /* a level ends with at most N_l + 2 nodes, except that the first pass splits all nIni initial nodes unconditionally (up
     * to 4 * nIni); the documented formula stays the floor so common configurations keep their layout */
    int bound = 0;
    for (int l = 0; l < nlevels; l++) {
        const int W = lw[l] - 2 * VSLAM_FAST_BORDER, H = lh[l] - 2 * VSLAM_FAST_BORDER;
        bound += std::max(quota[l] + 3, 4 * (int)std::round((float)W / (float)H));
    }
    return std::max((nfeatures + 4 * nlevels + 8 + 3) & ~3, (bound + 3) & ~3);
}

void plan_octree(const int* quota, const int* lw, const int* lh, const int* cell_first, int L, int forced_depth,
                 size_t budget, const std::function<size_t(int)>& node_bytes, OctPlan& P) {
    P = OctPlan();
    int maxNodes = 16, selOff = 0;
    bool fits = true;
    for (int l = 0; l < L; l++) {
        const int W = lw[l] - 2 * VSLAM_FAST_BORDER, H = lh[l] - 2 * VSLAM_FAST_BORDER;
        const int nIni = (int)std::round((float)W / (float)H);
        P.N[l] = quota[l];
        P.H[l] = H;
        P.nIni[l] = nIni;
        P.hX[l] = (float)W / nIni;
        P.selOff[l] = selOff;
        const int cap_l = std::max(P.N[l] + 3, 4 * nIni) + 1;
        selOff += cap_l;
        maxNodes = std::max(maxNodes, cap_l);
        /* at least one node per four cells of the level: k_octree_v4 borrows the node arrays behind the first one for the
         * level's cell offsets and segment bases (2 u32 per cell + sentinel; 10 u32 per node there).  The bound is looser
         * than v4 needs; it is kept as it is because v4's layout, fine depths and occupancy were measured with it */
        maxNodes = std::max(maxNodes, (cell_first[l + 1] - cell_first[l] + 1 + 3) / 4); /* + sentinel */
        if (nIni > 64) fits = false;
    }
    P.selStride = selOff;
    P.maxNodes = (maxNodes + 15) & ~15;
    /* k_octree_v4's fine grid: one level deeper than the depth at which a full quadtree has N nodes (nIni * 4^d
     * at depth d), so that the split passes, which stop at N nodes, mostly stay above it; keys that cluster
     * below it are handled exactly by the kernel's in-cell path, so the depth only decides speed.  Both arrays
     * of the largest level must fit LDS next to the node arrays (budget), and there are at most 16384 cells:
     * the kernel zeroes and scans both arrays once per problem, and that many cells are already 128 KB of LDS.
     * (The two-walk kernel also bounded the keys a cell can hold, for a 16-bit rank; nothing packs a rank now.)
     * forced_depth forces a depth where it is admissible (tests: deep splits everywhere). */
    const size_t nb = (node_bytes(P.maxNodes) + 15) & ~(size_t)15;
    int maxcells = 0;
    for (int l = 0; l < L; l++) {
        const int W = lw[l] - 2 * VSLAM_FAST_BORDER, H = P.H[l], nIni = P.nIni[l];
        int D = 1;
        while ((nIni << (2 * D)) < P.N[l]) D++;
        D += 1;
        if (forced_depth >= 0) D = forced_depth;
        D = std::max(1, std::min(D, 11));
        while (D > 1 && (((long long)nIni << (2 * D)) > 16384 || nb + 2 * (((size_t)nIni << (2 * D)) + 1) * 4 + 16 > budget))
            D--;
        P.fineD[l] = D;
        maxcells = std::max(maxcells, nIni << (2 * D));
        std::vector<uint32_t> xs, ys;
        build_oct_lut(W, H, D, xs, ys);
        P.lutOff[l] = (int32_t)P.lut.size();
        P.lutW[l] = (int32_t)xs.size();
        P.lut.insert(P.lut.end(), xs.begin(), xs.end());
        P.lut.insert(P.lut.end(), ys.begin(), ys.end());
    }
    P.fineLdsOff = (int32_t)nb;
    P.fineLdsBytes = (int32_t)(2 * ((size_t)maxcells + 1) * 4 + 16);
    /* depth 1 is the floor even over the budget, so the verdict is checked, not assumed: the whole allocation within a CU's
     * 160 KB and the node arrays within 150 KB of them (a list that does not fit LDS: host quadtree) */
    P.fits = fits && nb + (size_t)P.fineLdsBytes <= 160 * 1024 && node_bytes(P.maxNodes) <= 150 * 1024;
}

void build_oct_lut(int W, int H, int D, std::vector<uint32_t>& xs, std::vector<uint32_t>& ys) {
    const int nIni = (int)std::round((float)W / (float)H);
    const float hX = (float)W / (float)nIni;
    xs.assign((size_t)W + 1, 0u);
    ys.assign((size_t)H + 1, 0u);
    for (int x = 0; x <= W; x++) {
        int b = (int)((float)x / hX);
        b = std::min(b, nIni - 1);
        int x0 = (int)(hX * (float)b), x1 = (int)(hX * (float)(b + 1));
        uint32_t code = 0;
        for (int d = 0; d < D; d++) {
            const int mx = x0 + ((x1 - x0 + 1) >> 1);
            const int q = x < mx ? 0 : 1;
            code = (code << 2) | (uint32_t)q;
            if (q) x0 = mx; else x1 = mx;
        }
        xs[x] = ((uint32_t)b << (2 * D)) | code;
    }
    for (int y = 0; y <= H; y++) {
        int y0 = 0, y1 = H;
        uint32_t code = 0;
        for (int d = 0; d < D; d++) {
            const int my = y0 + ((y1 - y0 + 1) >> 1);
            const int q = y < my ? 0 : 1;
            code = (code << 2) | ((uint32_t)q << 1);
            if (q) y0 = my; else y1 = my;
        }
        ys[y] = code;
    }
}

void FrameGrid::build(const vslam_kp* k, int n_, int imgW, int imgH) {
    const float b[4] = {0.0f, (float)imgW, 0.0f, (float)imgH}; /* frame.cpp:814-820 */
    build(k, n_, b);
}

void FrameGrid::build(const vslam_kp* k, int n_, const float bounds[4]) {
    kps = k;
    n = n_;
    minX = bounds[0]; maxX = bounds[1]; minY = bounds[2]; maxY = bounds[3]; /* frame.cpp:793-821 */
    invW = (float)COLS / (maxX - minX);                                /* frame.cpp:322-323 */
    invH = (float)ROWS / (maxY - minY);
    std::vector<int> cellOf(n, -1);
    cell_start.assign(COLS * ROWS + 1, 0);
    for (int i = 0; i < n; i++) { /* PosInGrid, frame.cpp:746-756 */
        const int px = (int)std::round((k[i].x - minX) * invW);
        const int py = (int)std::round((k[i].y - minY) * invH);
        if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
        cellOf[i] = px * ROWS + py;
        cell_start[cellOf[i] + 1]++;
    }
    for (int cidx = 0; cidx < COLS * ROWS; cidx++) cell_start[cidx + 1] += cell_start[cidx];
    cell_items.resize(cell_start[COLS * ROWS]);
    std::vector<int> w(cell_start.begin(), cell_start.end() - 1);
    for (int i = 0; i < n; i++)
        if (cellOf[i] >= 0) cell_items[w[cellOf[i]]++] = i; /* ascending index inside a cell */
}

void FrameGrid::query(float x, float y, float r, int minLevel, int maxLevel, std::vector<int>& out) const {
    out.clear(); /* frame.cpp:678-744 */
    const int nMinCellX = std::max(0, (int)std::floor((x - minX - r) * invW));
    if (nMinCellX >= COLS) return;
    const int nMaxCellX = std::min(COLS - 1, (int)std::ceil((x - minX + r) * invW));
    if (nMaxCellX < 0) return;
    const int nMinCellY = std::max(0, (int)std::floor((y - minY - r) * invH));
    if (nMinCellY >= ROWS) return;
    const int nMaxCellY = std::min(ROWS - 1, (int)std::ceil((y - minY + r) * invH));
    if (nMaxCellY < 0) return;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
            const int cidx = ix * ROWS + iy;
            for (int e = cell_start[cidx]; e < cell_start[cidx + 1]; e++) {
                const int idx = cell_items[e];
                const vslam_kp& kp = kps[idx];
                if (bCheckLevels) {
                    if (kp.octave < minLevel) continue;
                    if (maxLevel >= 0 && kp.octave > maxLevel) continue;
                }
                const float distx = kp.x - x, disty = kp.y - y;
                if (std::fabs(distx) < r && std::fabs(disty) < r) out.push_back(idx);
            }
        }
}

int search_for_initialization_replay(const vslam_kp* kps1, int n1, const vslam_kp* kps2, int n2,
                                     const uint8_t* dmat, const int* row_of_i1, const int* col_of_i2,
                                     int ncols, const float bounds[4], float* prevMatched, int32_t* vnMatches12,
                                     int windowSize, float mfNNratio, bool checkOri) {
    /* fmatcher.cpp:983-1098 */
    const int TH_LOW = 50, HISTO_LENGTH = VSLAM_HISTO_LENGTH;
    int nmatches = 0;
    for (int i = 0; i < n1; i++) vnMatches12[i] = -1;
    std::vector<int> rotHist[HISTO_LENGTH];
    std::vector<int> vMatchedDistance(n2, INT_MAX), vnMatches21(n2, -1);
    FrameGrid grid2;
    grid2.build(kps2, n2, bounds);
    std::vector<int> vIndices2;
    for (int i1 = 0; i1 < n1; i1++) {
        const int level1 = kps1[i1].octave;
        if (level1 > 0) continue;
        grid2.query(prevMatched[2 * i1], prevMatched[2 * i1 + 1], (float)windowSize, level1, level1, vIndices2);
        if (vIndices2.empty()) continue;
        const uint8_t* drow = dmat + (size_t)row_of_i1[i1] * ncols;
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int i2 : vIndices2) {
            const int dist = drow[col_of_i2[i2]];
            if (vMatchedDistance[i2] <= dist) continue;
            if (dist < bestDist) {
                bestDist2 = bestDist;
                bestDist = dist;
                bestIdx2 = i2;
            } else if (dist < bestDist2) {
                bestDist2 = dist;
            }
        }
        if (bestDist <= TH_LOW) {
            if (bestDist < (float)bestDist2 * mfNNratio) {
                if (vnMatches21[bestIdx2] >= 0) {
                    vnMatches12[vnMatches21[bestIdx2]] = -1;
                    nmatches--;
                }
                vnMatches12[i1] = bestIdx2;
                vnMatches21[bestIdx2] = i1;
                vMatchedDistance[bestIdx2] = bestDist;
                nmatches++;
                if (checkOri) rotHist[vslam_md::rot_bin(kps1[i1].angle, kps2[bestIdx2].angle, HISTO_LENGTH)].push_back(i1);
            }
        }
    }
    if (checkOri) {
        int sizes[HISTO_LENGTH];
        for (int i = 0; i < HISTO_LENGTH; i++) sizes[i] = (int)rotHist[i].size();
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(sizes, HISTO_LENGTH); /* the kernels' text (vslam_matchdev.h) */
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (vslam_md::keeps_bin(mx, i)) continue;
            for (int idx1 : rotHist[i])
                if (vnMatches12[idx1] >= 0) {
                    vnMatches12[idx1] = -1;
                    nmatches--;
                }
        }
    }
    for (int i1 = 0; i1 < n1; i1++)
        if (vnMatches12[i1] >= 0) {
            prevMatched[2 * i1] = kps2[vnMatches12[i1]].x;
            prevMatched[2 * i1 + 1] = kps2[vnMatches12[i1]].y;
        }
    return nmatches;
}

size_t layout_parts(size_t align, const size_t* sizes, int n, size_t* off) {
    size_t end = 0;
    for (int i = 0; i < n; i++) {
        off[i] = end;
        end = (end + sizes[i] + align - 1) & ~(align - 1);
    }
    return end;
}

} // namespace vslam

/* ---------------------------------------------------------------------------------------------
 * C hooks for the CPU test-suite (libvslam_host.so); not part of the product ABI.
 * ------------------------------------------------------------------------------------------- */
extern "C" {

int vslamh_tables(int nfeatures, float scale, int nlevels, float* sf, float* isf, float* s2, float* is2,
                  int* quota, int* umax16, int* disc_n) {
    vslam::ExtractorTables t;
    vslam::build_tables(nfeatures, scale, nlevels, t);
    for (int i = 0; i < nlevels; i++) {
        sf[i] = t.scale[i]; isf[i] = t.inv_scale[i]; s2[i] = t.sigma2[i]; is2[i] = t.inv_sigma2[i];
        quota[i] = t.quota[i];
    }
    for (int i = 0; i < 16; i++) umax16[i] = t.umax[i];
    *disc_n = (int)t.disc_u.size();
    return 0;
}

int vslamh_level_size(int nfeatures, float scale, int nlevels, int w, int h, int level, int* lw, int* lh) {
    vslam::ExtractorTables t;
    vslam::build_tables(nfeatures, scale, nlevels, t);
    vslam::level_size(t, w, h, level, lw, lh);
    return 0;
}

/* CPU evaluation of the resize tables exactly as k_resize_level consumes them */
int vslamh_resize_with_tables(const uint8_t* src, int sw, int sh, size_t sstride, uint8_t* dst, int dw, int dh,
                              size_t dstride) {
    vslam::ResizeTables r;
    vslam::build_resize_tables(sw, sh, dw, dh, r);
    for (int dy = 0; dy < dh; dy++)
        for (int dx = 0; dx < dw; dx++) {
            const uint8_t* r0 = src + (size_t)r.ytab[2 * dy] * sstride;
            const uint8_t* r1 = src + (size_t)r.ytab[2 * dy + 1] * sstride;
            const int sx0 = r.xtab[2 * dx], sx1 = r.xtab[2 * dx + 1], a0 = r.xa[2 * dx], a1 = r.xa[2 * dx + 1];
            const int h0 = r0[sx0] * a0 + r0[sx1] * a1, h1 = r1[sx0] * a0 + r1[sx1] * a1;
            const int b0 = r.yb[2 * dy], b1 = r.yb[2 * dy + 1];
            dst[(size_t)dy * dstride + dx] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
    return 0;
}

/* The fused pyramid plan evaluated on the CPU: builds the tables and group plans exactly as vslam_fe_create does
 * (groups of levels 1-3, 4-7, ...) and runs emulate_pyramid_group.  out = all levels >= 1 back to back, level l at
 * offset sum of w*h of the levels before it, tightly packed.  Returns the number of groups, or a negative code.
 * recs (may be null): one row of 16 int32 per (group, tile, entry j) -- group, tile, j, nl, c0, nc, r0, nr, sq0, sq1, sr0,
 * sr1, lds_off, pitch, rt_off, the plan's lds_bytes -- at most recs_cap rows; *nrecs = rows the plan has. */
static int pyramid_fused_with(const uint8_t* img, int w, int h, size_t stride, int nfeatures, float scale, int nlevels,
                              int rows, bool pingpong, size_t max_lds, uint8_t* out, int* lds_bytes_max, int* tiles_total,
                              int32_t* recs, int recs_cap, int* nrecs) {
    vslam::ExtractorTables t;
    vslam::build_tables(nfeatures, scale, nlevels, t);
    std::vector<vslam::PyrLevelTables> tabs(nlevels);
    std::vector<int> lw(nlevels), lh(nlevels);
    for (int l = 0; l < nlevels; l++) vslam::level_size(t, w, h, l, &lw[l], &lh[l]);
    for (int l = 1; l < nlevels; l++) {
        vslam::PyrLevelTables& T = tabs[l];
        T.sw = lw[l - 1]; T.sh = lh[l - 1]; T.dw = lw[l]; T.dh = lh[l];
        vslam::build_resize_tables(T.sw, T.sh, T.dw, T.dh, T.r);
        if (!vslam::build_resize_quads(T.r, T.sw, T.dw, T.qbase, T.quads)) return -100;
    }
    /* level images with the product's pitch (multiple of 128) */
    std::vector<std::vector<uint8_t>> lv(nlevels);
    std::vector<int> pitch(nlevels);
    for (int l = 0; l < nlevels; l++) {
        pitch[l] = (lw[l] + 127) & ~127;
        lv[l].assign((size_t)pitch[l] * lh[l], 0xEE);
    }
    for (int y = 0; y < h; y++) memcpy(&lv[0][(size_t)y * pitch[0]], img + (size_t)y * stride, w);
    int ngroups = 0, nr = 0;
    *lds_bytes_max = 0;
    *tiles_total = 0;
    for (int l0 = 0; l0 + 1 < nlevels;) {
        const int nl = std::min(l0 == 0 ? 3 : 4, nlevels - 1 - l0);
        std::vector<const vslam::PyrLevelTables*> gt;
        for (int j = 1; j <= nl; j++) gt.push_back(&tabs[l0 + j]);
        vslam::PyrGroupPlan plan;
        if (!vslam::build_pyramid_group(gt, l0, max_lds, plan, rows, pingpong)) return -101;
        std::vector<uint8_t*> dst(nl + 1, nullptr);
        std::vector<int> ds(nl + 1, 0);
        for (int j = 1; j <= nl; j++) { dst[j] = lv[l0 + j].data(); ds[j] = pitch[l0 + j]; }
        /* level 0 may be the caller's image (readable up to w only); internal levels are readable up to their pitch */
        const int rc = vslam::emulate_pyramid_group(plan, gt, lv[l0].data(), pitch[l0], l0 == 0 ? w : pitch[l0], dst, ds);
        if (rc) return rc;
        for (int tile = 0; tile < plan.ntx * plan.nty; tile++)
            for (int j = 0; j <= nl; j++, nr++) {
                if (!recs || nr >= recs_cap) continue;
                const vslam::PyrTileLevel& T = plan.tiles[(size_t)tile * (nl + 1) + j];
                const int32_t row[16] = {ngroups, tile, j, nl, T.c0, T.nc, T.r0, T.nr, T.sq0, T.sq1, T.sr0, T.sr1,
                                         (int32_t)T.lds_off, (int32_t)T.pitch, (int32_t)T.rt_off, (int32_t)plan.lds_bytes};
                memcpy(recs + (size_t)nr * 16, row, sizeof(row));
            }
        *lds_bytes_max = std::max(*lds_bytes_max, (int)plan.lds_bytes);
        *tiles_total += plan.ntx * plan.nty;
        ngroups++;
        l0 += nl;
    }
    if (nrecs) *nrecs = nr;
    size_t o = 0;
    for (int l = 1; l < nlevels; l++)
        for (int y = 0; y < lh[l]; y++) {
            memcpy(out + o, &lv[l][(size_t)y * pitch[l]], lw[l]);
            o += lw[l];
        }
    return ngroups;
}

int vslamh_pyramid_fused(const uint8_t* img, int w, int h, size_t stride, int nfeatures, float scale, int nlevels,
                         uint8_t* out, int* lds_bytes_max, int* tiles_total) {
    return pyramid_fused_with(img, w, h, stride, nfeatures, scale, nlevels, -1, false, 64 * 1024, out, lds_bytes_max, tiles_total,
                              nullptr, 0, nullptr);
}

/* The same with the tile shape a context of `batch` images gets from vslam_tuning.pyr_rows / pyr_pingpong (-1: default),
 * and with the plan's tile records (see pyramid_fused_with).  *shape = {rows, pingpong, LDS limit} as resolved. */
int vslamh_pyramid_fused_shape(const uint8_t* img, int w, int h, size_t stride, int nfeatures, float scale, int nlevels, int batch,
                               int tune_rows, int tune_pingpong, uint8_t* out, int* lds_bytes_max, int* tiles_total, int32_t* shape,
                               int32_t* recs, int recs_cap, int* nrecs) {
    int rows;
    bool pingpong;
    size_t max_lds;
    vslam::pyramid_tile_shape(w, h, batch, tune_rows, tune_pingpong, &rows, &pingpong, &max_lds);
    if (shape) { shape[0] = rows; shape[1] = pingpong; shape[2] = (int32_t)max_lds; }
    return pyramid_fused_with(img, w, h, stride, nfeatures, scale, nlevels, rows, pingpong, max_lds, out, lds_bytes_max, tiles_total,
                              recs, recs_cap, nrecs);
}

int vslamh_cells(int level, int lw, int lh, uint16_t* out5, int cap) {
    std::vector<vslam::HostCell> c;
    vslam::build_cells(level, lw, lh, c);
    for (int i = 0; i < (int)c.size() && i < cap; i++) {
        out5[5 * i] = c[i].level; out5[5 * i + 1] = c[i].x0; out5[5 * i + 2] = c[i].y0;
        out5[5 * i + 3] = c[i].x1; out5[5 * i + 4] = c[i].y1;
    }
    return (int)c.size();
}

/* bands of all cells of one level: out8 rows = (cell0, level, ncell, wcell, x0, y0, ww, wh) */
int vslamh_bands(int level, int lw, int lh, int max_cells, int max_width, uint32_t* out8, int cap) {
    std::vector<vslam::HostCell> c;
    vslam::build_cells(level, lw, lh, c);
    std::vector<vslam::HostBand> b;
    vslam::build_bands(c, max_cells, max_width, b);
    for (int i = 0; i < (int)b.size() && i < cap; i++) {
        uint32_t* o = out8 + 8 * i;
        o[0] = b[i].cell0; o[1] = b[i].level; o[2] = b[i].ncell; o[3] = b[i].wcell;
        o[4] = b[i].x0; o[5] = b[i].y0; o[6] = b[i].ww; o[7] = b[i].wh;
    }
    return (int)b.size();
}

/* keys: n x (x, y, response) int32 triples; returns count, writes triples */
int vslamh_octree(const int32_t* xyr, int n, int W, int H, int N, int32_t* out_xyr, int cap) {
    std::vector<vslam::Cand> c(n), o;
    for (int i = 0; i < n; i++) {
        c[i].x = (int16_t)xyr[3 * i]; c[i].y = (int16_t)xyr[3 * i + 1]; c[i].response = (uint8_t)xyr[3 * i + 2];
    }
    if (!vslam::distribute_octree(c.data(), n, W, H, N, o)) return -1;
    for (int i = 0; i < (int)o.size() && i < cap; i++) {
        out_xyr[3 * i] = o[i].x; out_xyr[3 * i + 1] = o[i].y; out_xyr[3 * i + 2] = o[i].response;
    }
    return (int)o.size();
}

int vslamh_grid_query(const vslam_kp* kps, int n, int W, int H, float x, float y, float r, int minL, int maxL,
                      int* out, int cap) {
    vslam::FrameGrid g;
    g.build(kps, n, W, H);
    std::vector<int> v;
    g.query(x, y, r, minL, maxL, v);
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}

/* dense host replay with a caller-provided full n1 x n2 u8 distance matrix */
int vslamh_search_init(const vslam_kp* kps1, int n1, const vslam_kp* kps2, int n2, const uint8_t* dmat_full,
                       int W, int H, float* prevMatched, int32_t* matches12, int window, float nnratio,
                       int checkOri) {
    std::vector<int> rows(n1), cols(n2);
    for (int i = 0; i < n1; i++) rows[i] = i;
    for (int i = 0; i < n2; i++) cols[i] = i;
    const float b[4] = {0.0f, (float)W, 0.0f, (float)H};
    return vslam::search_for_initialization_replay(kps1, n1, kps2, n2, dmat_full, rows.data(), cols.data(), n2,
                                                   b, prevMatched, matches12, window, nnratio, checkOri != 0);
}

/* the same over float grid bounds (minX, maxX, minY, maxY): the host replay of the _ex entry points */
int vslamh_search_init_bounds(const vslam_kp* kps1, int n1, const vslam_kp* kps2, int n2, const uint8_t* dmat_full,
                              const float* bounds, float* prevMatched, int32_t* matches12, int window, float nnratio,
                              int checkOri) {
    std::vector<int> rows(n1), cols(n2);
    for (int i = 0; i < n1; i++) rows[i] = i;
    for (int i = 0; i < n2; i++) cols[i] = i;
    return vslam::search_for_initialization_replay(kps1, n1, kps2, n2, dmat_full, rows.data(), cols.data(), n2,
                                                   bounds, prevMatched, matches12, window, nnratio, checkOri != 0);
}

/* cv::undistortPoints as Frame::UndistortKeyPoints applies it (k1 == 0: unchanged), the shared vslam_undistort.h code:
 * cam = fx, fy, cx, cy; dist = ndist (4 or 5) coefficients; xy / out = n interleaved points */
int vslamh_undistort_points(const float* cam, const float* dist, int ndist, const float* xy, int n, float* out) {
    if (ndist != 4 && ndist != 5) return -1;
    float d[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; i++) d[i] = dist[i];
    for (int i = 0; i < n; i++) vslam_ud::frame_undistort(xy[2 * i], xy[2 * i + 1], cam, d, &out[2 * i], &out[2 * i + 1]);
    return 0;
}

/* Frame::ComputeImageBounds of a cols x rows image: minX, maxX, minY, maxY */
int vslamh_image_bounds(const float* cam, const float* dist, int ndist, int cols, int rows, float* b) {
    if (ndist != 4 && ndist != 5) return -1;
    float d[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; i++) d[i] = dist[i];
    vslam_ud::image_bounds(cam, d, cols, rows, b);
    return 0;
}

/* Frame::isInFrustum over n MapPoints, the shared vslam_frustum.h code (CPU tests, the stand-alone demo; the product runs
 * k_frustum).  Beside the parameters and the points it takes what the product reads from its context: the grid bounds in
 * force (bounds = minX, maxX, minY, maxY or NULL for {0, img_w, 0, img_h}) and the extractor's level count (the clamp of
 * PredictScale); depth_out may be NULL.  Returns nToMatch,
 * -1 for bad arguments. */
int vslamh_in_frustum(const vslam_frustum_params* p, const float* bounds, int nlevels, const vslam_map_point* points, int n,
                      vslam_mp_track* track_out, float* depth_out) {
    if (!p || n < 0 || nlevels < 1 || (n && (!points || !track_out))) return -1;
    const float whole[4] = {0.0f, (float)p->img_w, 0.0f, (float)p->img_h};
    const vslam_fr::Frame F = vslam_fr::make_frame(*p, bounds ? bounds : whole, nlevels);
    int in_view = 0;
    for (int i = 0; i < n; i++) {
        float depth;
        vslam_fr::in_frustum(F, points[i], &track_out[i], &depth);
        if (depth_out) depth_out[i] = depth;
        in_view += (int)(track_out[i].flags & 1u);
    }
    return in_view;
}

/* The host end of vslam_search_local_points_wait: the matcher ran on the compacted list, so match_compact[idx] counts kept
 * points; orig_index[k] is the k-th kept point's index in the caller's array.  More kept points than the matcher's capacity:
 * nothing can be said about any keypoint -- all -1 and VSLAM_ERR_UNSUPPORTED. */
int vslamh_local_points_finish(const int32_t* match_compact, int n_cur, const int32_t* orig_index, int n_kept, int capacity,
                               int32_t* match_cur) {
    if (n_cur < 0 || n_kept < 0 || capacity < 0 || (n_cur && (!match_compact || !match_cur)) || (n_kept && !orig_index))
        return VSLAM_ERR_INVALID;
    if (n_kept > capacity) {
        for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
        return VSLAM_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < n_cur; i++) {
        const int32_t k = match_compact[i];
        match_cur[i] = (k >= 0 && k < n_kept) ? orig_index[k] : -1;
    }
    return VSLAM_OK;
}

/* mvLeftToRightMatch / mvRightToLeftMatch of a rig frame: every entry -1 or an index of the other side */
int vslamh_rig_maps_check(const int32_t* left_to_right, int n_left, const int32_t* right_to_left, int n_right) {
    if (n_left < 0 || n_right < 0 || (n_left && !left_to_right) || (n_right && !right_to_left)) return VSLAM_ERR_INVALID;
    for (int i = 0; i < n_left; i++)
        if (left_to_right[i] < -1 || left_to_right[i] >= n_right) return VSLAM_ERR_INVALID;
    for (int i = 0; i < n_right; i++)
        if (right_to_left[i] < -1 || right_to_left[i] >= n_left) return VSLAM_ERR_INVALID;
    return VSLAM_OK;
}

namespace {
/* Frame::AssignFeaturesToGrid / PosInGrid (frame.cpp:322-323, :746-756) and GetFeaturesInArea (:678-744) over one keypoint set */
struct RigGrid {
    static const int COLS = 64, ROWS = 48;
    const vslam_kp* kps;
    float minX, minY, invW, invH;
    std::vector<std::vector<int>> cell;
    RigGrid(const vslam_kp* k, int n, const float* b) : kps(k), cell((size_t)COLS * ROWS) {
        minX = b[0];
        minY = b[2];
        invW = (float)COLS / (b[1] - b[0]);
        invH = (float)ROWS / (b[3] - b[2]);
        for (int i = 0; i < n; i++) {
            const int px = (int)roundf((k[i].x - minX) * invW), py = (int)roundf((k[i].y - minY) * invH);
            if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
            cell[(size_t)px * ROWS + py].push_back(i);
        }
    }
    void query(float x, float y, float r, int minLevel, int maxLevel, std::vector<int>& out) const {
        out.clear();
        const int c0 = std::max(0, (int)floorf((x - minX - r) * invW));
        if (c0 >= COLS) return;
        const int c1 = std::min(COLS - 1, (int)ceilf((x - minX + r) * invW));
        if (c1 < 0) return;
        const int r0 = std::max(0, (int)floorf((y - minY - r) * invH));
        if (r0 >= ROWS) return;
        const int r1 = std::min(ROWS - 1, (int)ceilf((y - minY + r) * invH));
        if (r1 < 0) return;
        const bool check = minLevel > 0 || maxLevel >= 0;
        for (int ix = c0; ix <= c1; ix++)
            for (int iy = r0; iy <= r1; iy++)
                for (int i : cell[(size_t)ix * ROWS + iy]) {
                    if (check) {
                        if (kps[i].octave < minLevel) continue;
                        if (maxLevel >= 0 && kps[i].octave > maxLevel) continue;
                    }
                    if (fabsf(kps[i].x - x) < r && fabsf(kps[i].y - y) < r) out.push_back(i);
                }
    }
};
int rig_hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}
struct RigBest {
    int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
    void take(int dist, int level, int idx) { /* fmatcher.cpp:381-397 */
        if (dist < bestDist) {
            bestDist2 = bestDist;
            bestDist = dist;
            bestLevel2 = bestLevel;
            bestLevel = level;
            bestIdx = idx;
        } else if (dist < bestDist2) {
            bestLevel2 = level;
            bestDist2 = dist;
        }
    }
};
} // namespace

/* FMatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th, ...) (fmatcher.cpp:321-491) as it is written, for both
 * kinds of Frame; the sequential statement the device resolver (k_rig_resolve) is tested against, CPU tests and the demo.
 * track_right == NULL: Nleft == -1 (the right arguments are not read; u_right, may be NULL, is the frame's mvuRight).
 * Otherwise a rig: slots [0, n_left) are the left keypoints, [n_left, n_left + n_right) the right ones.  Records as
 * Frame::isInFrustum leaves them, far test and isBad folded into flag bit 0; bit 1 (of either record) = Observations() > 0.
 * scale_factors: mvScaleFactors, nlevels entries; bounds: mnMinX, mnMaxX, mnMinY, mnMaxY.  occupied (may be NULL): per slot. */
int vslamh_search_by_projection_mappoints_rig(const vslam_mp_track* track_left, const vslam_mp_track* track_right,
                                              const uint8_t* mp_desc, int n_mp, const vslam_kp* kps_left,
                                              const uint8_t* desc_left, int n_left, const vslam_kp* kps_right,
                                              const uint8_t* desc_right, int n_right, const int32_t* left_to_right,
                                              const int32_t* right_to_left, const float* u_right, const uint8_t* occupied,
                                              const float* scale_factors, int nlevels, const float* bounds, float th,
                                              float nnratio, int32_t* match_cur, int* nmatches) {
    const bool rig = track_right != nullptr;
    if (!rig) n_right = 0;
    if (n_mp < 0 || n_left < 0 || n_right < 0 || nlevels < 1 || !scale_factors || !bounds || !nmatches ||
        (n_mp && (!track_left || !mp_desc)) || (n_left && (!kps_left || !desc_left)) || (n_right && (!kps_right || !desc_right)) ||
        ((n_left + n_right) && !match_cur))
        return VSLAM_ERR_INVALID;
    if (rig)
        if (int rc = vslamh_rig_maps_check(left_to_right, n_left, right_to_left, n_right)) return rc;
    const int TH_HIGH = 100;
    const int N = n_left + n_right;
    std::vector<uint8_t> occ((size_t)N, 0);
    for (int i = 0; i < N; i++) {
        match_cur[i] = -1;
        if (occupied) occ[i] = occupied[i] != 0;
    }
    const RigGrid gl(kps_left, n_left, bounds), gr(kps_right, n_right, bounds);
    std::vector<int> vIndices;
    const bool bFactor = th != 1.0f;
    int nm = 0;
    /* mvScaleFactors[level]: a caller-made record's level is clamped into the table, as k_sbp_rank does */
    auto scale_of = [&](int l) { return scale_factors[std::min(std::max(l, 0), nlevels - 1)]; };
    for (int iMP = 0; iMP < n_mp; iMP++) {
        const vslam_mp_track& L = track_left[iMP];
        const bool inL = (L.flags & 1u) != 0, inR = rig && (track_right[iMP].flags & 1u) != 0;
        if (!inL && !inR) continue;
        const uint8_t obs = ((L.flags | (rig ? track_right[iMP].flags : 0u)) & 2u) ? 1 : 0;
        const uint8_t* d = mp_desc + (size_t)iMP * 32;
        if (inL) {
            float r = (double)L.view_cos > 0.998 ? 2.5f : 4.0f;
            if (bFactor) r *= th;
            const float rs = r * scale_of(L.level);
            gl.query(L.proj_x, L.proj_y, rs, L.level - 1, L.level, vIndices);
            if (!vIndices.empty()) {
                RigBest b;
                for (int idx : vIndices) {
                    if (occ[idx]) continue;
                    if (!rig && u_right && u_right[idx] > 0) {
                        const float er = fabsf(L.proj_xr - u_right[idx]);
                        if (er > rs) continue;
                    }
                    b.take(rig_hamming(d, desc_left + (size_t)idx * 32), kps_left[idx].octave, idx);
                }
                if (b.bestDist <= TH_HIGH) {
                    if (b.bestLevel == b.bestLevel2 && (float)b.bestDist > nnratio * (float)b.bestDist2) continue;
                    match_cur[b.bestIdx] = iMP;
                    occ[b.bestIdx] = obs;
                    if (rig && left_to_right[b.bestIdx] != -1) {
                        const int s = left_to_right[b.bestIdx] + n_left;
                        match_cur[s] = iMP;
                        occ[s] = obs;
                        nm++;
                    }
                    nm++;
                }
            }
        }
        if (inR) {
            const vslam_mp_track& R = track_right[iMP];
            if (R.level == -1) continue;
            const float r = (double)R.view_cos > 0.998 ? 2.5f : 4.0f; /* no bFactor here (fmatcher.cpp:425) */
            gr.query(R.proj_x, R.proj_y, r * scale_of(R.level), R.level - 1, R.level, vIndices);
            if (vIndices.empty()) continue;
            RigBest b;
            for (int idx : vIndices) {
                if (occ[idx + n_left]) continue;
                b.take(rig_hamming(d, desc_right + (size_t)idx * 32), kps_right[idx].octave, idx);
            }
            if (b.bestDist <= TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && (float)b.bestDist > nnratio * (float)b.bestDist2) continue;
                if (right_to_left[b.bestIdx] != -1) {
                    match_cur[right_to_left[b.bestIdx]] = iMP;
                    occ[right_to_left[b.bestIdx]] = obs;
                    nm++;
                }
                match_cur[b.bestIdx + n_left] = iMP;
                occ[b.bestIdx + n_left] = obs;
                nm++;
            }
        }
    }
    *nmatches = nm;
    return VSLAM_OK;
}

/* ---- fisheye cameras: the shared vslam_kb8.h code on the host (CPU tests, the stand-alone demo; the product runs the kernels
 * of vslam_kb8.hip) ---- */
/* the libm restatements over n arguments: fn 0 atanf, 1 tanf, 2 sinf, 3 cosf (a, out), 4 atan2f (a = y, b = x) */
int vslamh_libm_twin(int fn, const float* a, const float* b, int n, float* out) {
    if (fn < 0 || fn > 4 || n < 0 || (n && (!a || !out || (fn == 4 && !b)))) return -1;
    for (int i = 0; i < n; i++)
        out[i] = fn == 0 ? vslam_kb8::glibc_atanf(a[i]) : fn == 1 ? vslam_kb8::glibc_tanf(a[i])
               : fn == 2 ? vslam_trig::glibc_sinf(a[i]) : fn == 3 ? vslam_trig::glibc_cosf(a[i])
                         : vslam_kb8::glibc_atan2f(a[i], b[i]);
    return 0;
}
/* the PLATFORM libm over the same arguments, for comparing large samples without a foreign call per value */
int vslamh_libm_platform(int fn, const float* a, const float* b, int n, float* out) {
    if (fn < 0 || fn > 4 || n < 0 || (n && (!a || !out || (fn == 4 && !b)))) return -1;
    for (int i = 0; i < n; i++)
        out[i] = fn == 0 ? ::atanf(a[i]) : fn == 1 ? ::tanf(a[i]) : fn == 2 ? ::sinf(a[i]) : fn == 3 ? ::cosf(a[i])
                                                                                                    : ::atan2f(a[i], b[i]);
    return 0;
}
float vslamh_atanf(float x) { return vslam_kb8::glibc_atanf(x); }
float vslamh_atan2f(float y, float x) { return vslam_kb8::glibc_atan2f(y, x); }
float vslamh_tanf(float x) { return vslam_kb8::glibc_tanf(x); }
float vslamh_sinf(float x) { return vslam_trig::glibc_sinf(x); }
float vslamh_cosf(float x) { return vslam_trig::glibc_cosf(x); }

int vslamh_kb8_project(const vslam_kb8_camera* cam, const float* xyz, int n, float* uv) {
    if (!vslam_kb8::camera_ok(cam) || n < 0 || (n && (!xyz || !uv))) return -1;
    for (int i = 0; i < n; i++) {
        const vslam_kb8::Uv o = vslam_kb8::kb8_project(*cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        uv[2 * i] = o.u;
        uv[2 * i + 1] = o.v;
    }
    return 0;
}
/* steps (may be NULL): Newton steps taken per pixel, 0 where theta_d <= 1e-8 */
int vslamh_kb8_unproject(const vslam_kb8_camera* cam, const float* uv, int n, float* xyz, int32_t* steps) {
    if (!vslam_kb8::camera_ok(cam) || n < 0 || (n && (!uv || !xyz))) return -1;
    for (int i = 0; i < n; i++) {
        int st = 0;
        const vslam_kb8::Ray r = vslam_kb8::kb8_unproject(*cam, uv[2 * i], uv[2 * i + 1], &st);
        xyz[3 * i] = r.x;
        xyz[3 * i + 1] = r.y;
        xyz[3 * i + 2] = r.z;
        if (steps) steps[i] = st;
    }
    return 0;
}
/* vslamh_in_frustum with KannalaBrandt8::project; the intrinsics of p must equal the camera's.  Returns nToMatch, -1 for bad
 * arguments. */
int vslamh_in_frustum_kb8(const vslam_frustum_params* p, const vslam_kb8_camera* cam, const float* bounds, int nlevels,
                          const vslam_map_point* points, int n, vslam_mp_track* track_out, float* depth_out) {
    if (!p || !vslam_kb8::camera_ok(cam) || n < 0 || nlevels < 1 || (n && (!points || !track_out))) return -1;
    if (!vslam_kb8::intrinsics_match(*p, *cam)) return -1;
    const float whole[4] = {0.0f, (float)p->img_w, 0.0f, (float)p->img_h};
    const vslam_fr::Frame F = vslam_fr::make_frame(*p, bounds ? bounds : whole, nlevels);
    int in_view = 0;
    for (int i = 0; i < n; i++) {
        float depth;
        vslam_kb8::in_frustum_kb8(F, *cam, points[i], &track_out[i], &depth);
        if (depth_out) depth_out[i] = depth;
        in_view += (int)(track_out[i].flags & 1u);
    }
    return in_view;
}
/* vslam_frame_in_frustum_rig on the host: returns the number of points either camera sees, -1 for bad arguments */
int vslamh_in_frustum_kb8_rig(const vslam_frustum_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                              const float* bounds, int nlevels, const vslam_map_point* points, int n,
                              vslam_mp_track* track_left, vslam_mp_track* track_right, float* depth_left,
                              float* depth_right) {
    if (!p || !rig || !vslam_kb8::camera_ok(cam) || !vslam_kb8::camera_ok(&rig->cam2) || n < 0 || nlevels < 1 ||
        (n && (!points || !track_left || !track_right)))
        return -1;
    if (!vslam_kb8::intrinsics_match(*p, *cam)) return -1;
    const float whole[4] = {0.0f, (float)p->img_w, 0.0f, (float)p->img_h};
    const vslam_fr::Frame F = vslam_fr::make_frame(*p, bounds ? bounds : whole, nlevels);
    const vslam_kb8::RigRight R = vslam_kb8::rig_right(F, *rig);
    int in_view = 0;
    for (int i = 0; i < n; i++) {
        float dl, dr;
        const bool l = vslam_kb8::in_frustum_check(F, F.Tcw, F.Ow, *cam, points[i], &track_left[i], &dl);
        const bool r = vslam_kb8::in_frustum_check(F, R.T, R.twc, rig->cam2, points[i], &track_right[i], &dr);
        if (depth_left) depth_left[i] = dl;
        if (depth_right) depth_right[i] = dr;
        in_view += (int)(l || r);
    }
    return in_view;
}
int vslamh_kb8_exclusive(int other_set, float k1) { /* either way round: the other kind is set and the pinhole one distorts */
    return (other_set && k1 != 0.0f) ? VSLAM_ERR_INVALID : VSLAM_OK;
}
int vslamh_kb8_frustum_check(const vslam_frustum_params* p, const vslam_kb8_camera* cam) {
    if (!p) return VSLAM_ERR_INVALID;
    if (!cam) return VSLAM_OK;
    return vslam_kb8::intrinsics_match(*p, *cam) ? VSLAM_OK : VSLAM_ERR_INVALID;
}
int vslamh_kb8_projecting_entry(int has_kb8) { return has_kb8 ? VSLAM_ERR_UNSUPPORTED : VSLAM_OK; }
/* vslam_search_by_projection_frame_rig: fx, fy, cx, cy of the projection parameters equal the KB8 camera's bit for bit */
int vslamh_frame_rig_camera_check(const vslam_proj_params* p, const vslam_kb8_camera* cam) {
    if (!p || !cam) return VSLAM_ERR_INVALID;
    return (vslam_kb8::same_bits(p->fx, cam->fx) && vslam_kb8::same_bits(p->fy, cam->fy) && vslam_kb8::same_bits(p->cx, cam->cx) &&
            vslam_kb8::same_bits(p->cy, cam->cy))
               ? VSLAM_OK
               : VSLAM_ERR_INVALID;
}

namespace {
/* one row of R * x + t as ONE cv::gemm (double accumulation, rounded once), or in float */
float rig_gemm_row(const float* r, const float* x, float t, int flt) {
    if (!flt) {
        double s = (double)r[0] * (double)x[0];
        s = s + (double)r[1] * (double)x[1];
        s = s + (double)r[2] * (double)x[2];
        return (float)(s + (double)t);
    }
    float s = r[0] * x[0];
    s = s + r[1] * x[1];
    s = s + r[2] * x[2];
    return s + t;
}
void rig_transform(const float* T, const float* x, int flt, float* out) {
    for (int r = 0; r < 3; r++) out[r] = rig_gemm_row(T + 4 * r, x, T[4 * r + 3], flt);
}
} // namespace

/* FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) for a two-fisheye rig
 * (fmatcher.cpp:2494-2684 with CurrentFrame.Nleft != -1) as it is written, sequential: the statement the device form
 * (vslam_search_by_projection_frame_rig) is tested against, and the shim's fallback.  Same arguments with host keypoints;
 * cam = CurrentFrame.mpCamera, through which BOTH branches project; Trl = rows [R | t] of mTrl; scale_factors: mvScaleFactors,
 * nlevels entries; bounds: mnMinX, mnMaxX, mnMinY, mnMaxY; occupied (may be NULL): per slot of n_left + n_right. */
int vslamh_search_by_projection_frame_rig(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Trl,
                                          const vslam_kp* last_kps, int n_last, const uint8_t* last_flags, const float* last_x3dw,
                                          const uint8_t* mp_desc, const vslam_kp* kps_left, const uint8_t* desc_left, int n_left,
                                          const vslam_kp* kps_right, const uint8_t* desc_right, int n_right,
                                          const uint8_t* occupied, const float* scale_factors, int nlevels, const float* bounds,
                                          int32_t* match_cur, int* nmatches) {
    if (!p || !cam || !Trl || n_last < 0 || n_left < 0 || n_right < 0 || nlevels < 1 || !scale_factors || !bounds || !nmatches ||
        (n_last && (!last_kps || !last_flags || !last_x3dw || !mp_desc)) || (n_left && (!kps_left || !desc_left)) ||
        (n_right && (!kps_right || !desc_right)) || ((n_left + n_right) && !match_cur))
        return VSLAM_ERR_INVALID;
    if (vslamh_frame_rig_camera_check(p, cam)) return VSLAM_ERR_INVALID;
    const int TH_HIGH = 100, L = VSLAM_HISTO_LENGTH;
    const int N = n_left + n_right;
    std::vector<uint8_t> occ((size_t)N, 0);
    for (int i = 0; i < N; i++) {
        match_cur[i] = -1;
        if (occupied) occ[i] = occupied[i] != 0;
    }
    const RigGrid gl(kps_left, n_left, bounds), gr(kps_right, n_right, bounds);
    std::vector<int> vIndices2;
    std::vector<int> rotHist[VSLAM_HISTO_LENGTH];
    int nm = 0;
    for (int i = 0; i < n_last; i++) {
        if (!(last_flags[i] & 1)) continue; /* pMP && !LastFrame.mvbOutlier[i] */
        const uint8_t obs = (last_flags[i] & 2) ? 1 : 0;
        float x3Dc[3];
        rig_transform(p->Tcw, last_x3dw + 3 * i, p->gemm_float, x3Dc);
        const float invzc = (float)(1.0 / (double)x3Dc[2]);
        if (invzc < 0) continue;
        const vslam_kb8::Uv uv = vslam_kb8::kb8_project(*cam, x3Dc[0], x3Dc[1], x3Dc[2]);
        if (uv.u < bounds[0] || uv.u > bounds[1]) continue;
        if (uv.v < bounds[2] || uv.v > bounds[3]) continue;
        const int nLastOctave = last_kps[i].octave; /* keypoints_[i] | keypointsRight_[i - Nleft]: the caller's one array */
        const float radius = p->th * scale_factors[std::min(std::max(nLastOctave, 0), nlevels - 1)];
        const int minLevel = p->forward ? nLastOctave : p->backward ? 0 : nLastOctave - 1;
        const int maxLevel = p->forward ? -1 : p->backward ? nLastOctave : nLastOctave + 1;
        gl.query(uv.u, uv.v, radius, minLevel, maxLevel, vIndices2);
        if (vIndices2.empty()) continue;
        const uint8_t* dMP = mp_desc + (size_t)i * 32;
        {
            int bestDist = 256, bestIdx2 = -1;
            for (int i2 : vIndices2) {
                if (occ[i2]) continue;
                const int dist = rig_hamming(dMP, desc_left + (size_t)i2 * 32);
                if (dist < bestDist) {
                    bestDist = dist;
                    bestIdx2 = i2;
                }
            }
            if (bestDist <= TH_HIGH) {
                match_cur[bestIdx2] = i;
                occ[bestIdx2] = obs;
                nm++;
                if (p->check_orientation)
                    rotHist[vslam_md::rot_bin(last_kps[i].angle, kps_left[bestIdx2].angle, L)].push_back(bestIdx2);
            }
        }
        { /* :2593-2658: no depth test, no in-frame test, no empty-window `continue`; the LEFT camera's model */
            float x3Dr[3];
            rig_transform(Trl, x3Dc, p->gemm_float, x3Dr);
            const vslam_kb8::Uv uvr = vslam_kb8::kb8_project(*cam, x3Dr[0], x3Dr[1], x3Dr[2]);
            gr.query(uvr.u, uvr.v, radius, minLevel, maxLevel, vIndices2);
            int bestDist = 256, bestIdx2 = -1;
            for (int i2 : vIndices2) {
                if (occ[i2 + n_left]) continue;
                const int dist = rig_hamming(dMP, desc_right + (size_t)i2 * 32);
                if (dist < bestDist) {
                    bestDist = dist;
                    bestIdx2 = i2;
                }
            }
            if (bestDist <= TH_HIGH) {
                match_cur[bestIdx2 + n_left] = i;
                occ[bestIdx2 + n_left] = obs;
                nm++;
                if (p->check_orientation)
                    rotHist[vslam_md::rot_bin(last_kps[i].angle, kps_right[bestIdx2].angle, L)].push_back(bestIdx2 + n_left);
            }
        }
    }
    if (p->check_orientation) {
        int histo[VSLAM_HISTO_LENGTH];
        for (int b = 0; b < L; b++) histo[b] = (int)rotHist[b].size();
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(histo, L);
        for (int b = 0; b < L; b++)
            if (!vslam_md::keeps_bin(mx, b))
                for (int s : rotHist[b]) {
                    match_cur[s] = -1;
                    nm--;
                }
    }
    *nmatches = nm;
    return VSLAM_OK;
}

/* The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame / a two-fisheye rig
 * (fmatcher.cpp:1918-2119; the Scw overload :2121-2243 as sim3 = 1) as it is written, job after job and point after point:
 * the statement the device form (vslam_fuse_search_rig) is tested against, and what the shim's walk calls with ONE point to
 * redo a search whose MapPoint descriptor was recomputed.  Same arguments; every pointer a HOST pointer, a job's dev_kps /
 * dev_desc included; any number of jobs and points.  cam = mpCamera, rig (may be NULL when no job has camera 1) gives
 * mpCamera2; scale_factors / inv_sigma2: mvScaleFactors / mvInvLevelSigma2, nlevels entries; bounds: the Frame's float mnMinX,
 * mnMaxX, mnMinY, mnMaxY, which the KeyFrame truncates for its window origin and IsInImage.  best_idx / best_dist: n_jobs *
 * n_points entries each, job-major. */
int vslamh_fuse_search_rig(const vslam_fuse_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                           const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points, const uint8_t* mp_desc,
                           int n_points, const float* scale_factors, const float* inv_sigma2, int nlevels, const float* bounds,
                           int32_t* best_idx, int32_t* best_dist) {
    if (!p || !vslam_kb8::camera_ok(cam) || !jobs || n_jobs < 1 || n_points < 0 || nlevels < 1 || !scale_factors || !inv_sigma2 ||
        !bounds || (n_points && (!points || !mp_desc || !best_idx || !best_dist)))
        return VSLAM_ERR_INVALID;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_fuse_rig_job& s = jobs[j];
        if (s.camera < 0 || s.camera > 1 || s.sim3 < 0 || s.sim3 > 1 || (s.sim3 && s.camera) || s.n_kf < 0 ||
            (s.n_kf && (!s.dev_kps || !s.dev_desc)) || (s.camera == 1 && (!rig || !vslam_kb8::camera_ok(&rig->cam2))))
            return VSLAM_ERR_INVALID;
    }
    const float kb[4] = {(float)(int)bounds[0], (float)(int)bounds[1], (float)(int)bounds[2], (float)(int)bounds[3]};
    std::vector<int> vIndices;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_fuse_rig_job& s = jobs[j];
        const vslam_kb8_camera& c = s.camera ? rig->cam2 : *cam;
        RigGrid grid(s.dev_kps, s.n_kf, bounds); /* the Frame's cells and inverses (keyframe.cpp:36, :58-67) .. */
        grid.minX = kb[0];                       /* .. the window origin from the KeyFrame's integers (:663-675) */
        grid.minY = kb[2];
        int32_t* bi = best_idx + (size_t)j * n_points;
        int32_t* bd = best_dist + (size_t)j * n_points;
        for (int i = 0; i < n_points; i++) {
            bi[i] = -1;
            bd[i] = 256;
            const vslam_fuse_point& mp = points[i];
            if (!mp.valid || (s.valid_host && !s.valid_host[i])) continue;
            float pc[3];
            for (int r = 0; r < 3; r++) pc[r] = rig_gemm_row(s.Rcw + 3 * r, mp.pos, s.tcw[r], p->gemm_float);
            if (pc[2] < 0.0f) continue;
            const vslam_kb8::Uv uv = vslam_kb8::kb8_project(c, pc[0], pc[1], pc[2]);
            if (!(uv.u >= kb[0] && uv.u < kb[1] && uv.v >= kb[2] && uv.v < kb[3])) continue; /* KeyFrame::IsInImage */
            const float p0 = mp.pos[0] - s.Ow[0], p1 = mp.pos[1] - s.Ow[1], p2 = mp.pos[2] - s.Ow[2];
            const float dist3D = vslam_md::norm3(p0, p1, p2);
            if (dist3D < mp.min_distance || dist3D > mp.max_distance) continue;
            if (vslam_md::dot3_mat(p0, p1, p2, mp.normal) < 0.5 * (double)dist3D) continue;
            const int level = vslam_md::predict_level(mp.max_distance, dist3D, p->log_scale_factor, nlevels);
            const float radius = p->th * scale_factors[level];
            grid.query(uv.u, uv.v, radius, -1, -1, vIndices);
            const uint8_t* dMP = mp_desc + (size_t)i * 32;
            int bestDist = s.sim3 ? INT_MAX : 256, bestIdx = -1;
            for (int idx : vIndices) {
                const int kpLevel = s.dev_kps[idx].octave;
                if (kpLevel < level - 1 || kpLevel > level) continue;
                if (!s.sim3) { /* mvuRight is -1 throughout: the monocular branch */
                    const float ex = uv.u - s.dev_kps[idx].x, ey = uv.v - s.dev_kps[idx].y;
                    const float e2 = ex * ex + ey * ey;
                    if ((double)(e2 * inv_sigma2[std::min(kpLevel, nlevels - 1)]) > 5.99) continue;
                }
                const int dist = rig_hamming(dMP, s.dev_desc + (size_t)idx * 32);
                if (dist < bestDist) {
                    bestDist = dist;
                    bestIdx = idx;
                }
            }
            if (bestIdx >= 0) {
                bi[i] = bestIdx + s.idx_offset;
                bd[i] = bestDist;
            }
        }
    }
    return VSLAM_OK;
}

/* FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (fmatcher.cpp:2689-2811) with a
 * fisheye CurrentFrame as it is written, sequential: the statement vslam_search_by_projection_keyframe_kb8 is tested against.
 * Same arguments with host keypoints; cam = CurrentFrame.mpCamera; cur_kps / cur_desc: keypoints_ and the descriptor rows
 * [0, n_cur), of a rig the LEFT camera's (bRight defaults to false); kf_kps: mvKeys followed by mvKeysRight -- the reference
 * reads pKF->mvKeysUn[i].angle past the end for i >= NLeft, the restatement the right keypoint's angle. */
int vslamh_search_by_projection_keyframe_kb8(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Ow,
                                             float log_scale_factor, int orb_dist, const vslam_kp* kf_kps, int n_kf,
                                             const uint8_t* mp_flags, const float* mp_x3dw, const float* mp_min_dist,
                                             const float* mp_max_dist, const uint8_t* mp_desc, const vslam_kp* cur_kps,
                                             const uint8_t* cur_desc, int n_cur, const uint8_t* cur_occupied,
                                             const float* scale_factors, int nlevels, const float* bounds, int32_t* match_cur,
                                             int* nmatches) {
    if (!p || !vslam_kb8::camera_ok(cam) || !Ow || n_kf < 0 || n_cur < 0 || nlevels < 1 || !scale_factors || !bounds || !nmatches ||
        orb_dist < 1 || orb_dist > 255 ||
        (n_kf && (!kf_kps || !mp_flags || !mp_x3dw || !mp_min_dist || !mp_max_dist || !mp_desc)) ||
        (n_cur && (!cur_kps || !cur_desc || !match_cur)))
        return VSLAM_ERR_INVALID;
    if (vslamh_frame_rig_camera_check(p, cam)) return VSLAM_ERR_INVALID;
    const int L = VSLAM_HISTO_LENGTH;
    std::vector<uint8_t> occ((size_t)n_cur, 0);
    for (int i = 0; i < n_cur; i++) {
        match_cur[i] = -1;
        if (cur_occupied) occ[i] = cur_occupied[i] != 0;
    }
    const RigGrid grid(cur_kps, n_cur, bounds);
    std::vector<int> vIndices2;
    std::vector<int> rotHist[VSLAM_HISTO_LENGTH];
    int nm = 0;
    for (int i = 0; i < n_kf; i++) {
        if (!(mp_flags[i] & 1)) continue; /* pMP && !pMP->isBad() && !sAlreadyFound.count(pMP) */
        const float* x3Dw = mp_x3dw + 3 * i;
        float x3Dc[3];
        rig_transform(p->Tcw, x3Dw, p->gemm_float, x3Dc);
        const vslam_kb8::Uv uv = vslam_kb8::kb8_project(*cam, x3Dc[0], x3Dc[1], x3Dc[2]); /* no depth test */
        if (uv.u < bounds[0] || uv.u > bounds[1]) continue;
        if (uv.v < bounds[2] || uv.v > bounds[3]) continue;
        const float dist3D = vslam_md::norm3(x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]);
        if (dist3D < mp_min_dist[i] || dist3D > mp_max_dist[i]) continue;
        const int level = vslam_md::predict_level(mp_max_dist[i], dist3D, log_scale_factor, nlevels);
        const float radius = p->th * scale_factors[level];
        grid.query(uv.u, uv.v, radius, level - 1, level + 1, vIndices2);
        if (vIndices2.empty()) continue;
        const uint8_t* dMP = mp_desc + (size_t)i * 32;
        int bestDist = 256, bestIdx2 = -1;
        for (int i2 : vIndices2) {
            if (occ[i2]) continue;
            const int dist = rig_hamming(dMP, cur_desc + (size_t)i2 * 32);
            if (dist < bestDist) {
                bestDist = dist;
                bestIdx2 = i2;
            }
        }
        if (bestDist <= orb_dist) {
            match_cur[bestIdx2] = i;
            occ[bestIdx2] = 1;
            nm++;
            if (p->check_orientation) rotHist[vslam_md::rot_bin(kf_kps[i].angle, cur_kps[bestIdx2].angle, L)].push_back(bestIdx2);
        }
    }
    if (p->check_orientation) {
        int histo[VSLAM_HISTO_LENGTH];
        for (int b = 0; b < L; b++) histo[b] = (int)rotHist[b].size();
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(histo, L);
        for (int b = 0; b < L; b++)
            if (!vslam_md::keeps_bin(mx, b))
                for (int s : rotHist[b]) {
                    match_cur[s] = -1;
                    nm--;
                }
    }
    *nmatches = nm;
    return VSLAM_OK;
}

/* FMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (fmatcher.cpp:750-863) for fisheye KeyFrames as
 * it is written, job after job and point after point: the statement vslam_search_by_projection_sim3_kb8 is tested against, and
 * what the shim runs for a job the device refused.  Same arguments; every pointer a HOST pointer, a job's dev_kps / dev_desc
 * included; any number of jobs, points and survivors.  n_gated[j] (may be NULL): the points that pass every gate up to the
 * radius.  bounds: the Frame's float mnMinX, mnMaxX, mnMinY, mnMaxY, truncated for the KeyFrame. */
int vslamh_search_by_projection_sim3_kb8(const vslam_sim3_kb8_params* p, const vslam_kb8_camera* cam,
                                         const vslam_sim3_kb8_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                         const uint8_t* mp_desc, int n_points, const float* scale_factors, int nlevels,
                                         const float* bounds, int32_t* const* match_kf, int* nmatches, int* n_gated) {
    if (!p || !vslam_kb8::camera_ok(cam) || !jobs || n_jobs < 1 || n_points < 0 || nlevels < 1 || !scale_factors || !bounds ||
        !match_kf || !nmatches || (n_points && (!points || !mp_desc)) || p->th < 0 || !(p->ratio_hamming >= 0.0f))
        return VSLAM_ERR_INVALID;
    for (int j = 0; j < n_jobs; j++)
        if (jobs[j].n_kf < 0 || (jobs[j].n_kf && (!jobs[j].dev_kps || !jobs[j].dev_desc || !match_kf[j]))) return VSLAM_ERR_INVALID;
    const float kb[4] = {(float)(int)bounds[0], (float)(int)bounds[1], (float)(int)bounds[2], (float)(int)bounds[3]};
    const float lim = 50 * p->ratio_hamming; /* bestDist <= TH_LOW * ratioHamming with an integer bestDist */
    const int thr = lim >= 255.0f ? 255 : std::max(0, (int)floorf(lim));
    const float th = (float)p->th;
    std::vector<int> vIndices;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_sim3_kb8_job& s = jobs[j];
        RigGrid grid(s.dev_kps, s.n_kf, bounds); /* the Frame's cells and inverses, the KeyFrame's integer window origin */
        grid.minX = kb[0];
        grid.minY = kb[2];
        std::vector<uint8_t> matched((size_t)s.n_kf, 0);
        for (int c = 0; c < s.n_kf; c++) {
            match_kf[j][c] = -1;
            if (s.kf_matched_host) matched[c] = s.kf_matched_host[c] != 0;
        }
        int nm = 0, gated = 0;
        for (int iMP = 0; iMP < n_points; iMP++) {
            const vslam_fuse_point& mp = points[iMP];
            if (!mp.valid || (s.valid_host && !s.valid_host[iMP])) continue;
            float pc[3];
            for (int r = 0; r < 3; r++) pc[r] = rig_gemm_row(s.Rcw + 3 * r, mp.pos, s.tcw[r], p->gemm_float);
            if (pc[2] < 0.0f) continue;
            const vslam_kb8::Uv uv = vslam_kb8::kb8_project(*cam, pc[0], pc[1], pc[2]);
            if (!(uv.u >= kb[0] && uv.u < kb[1] && uv.v >= kb[2] && uv.v < kb[3])) continue; /* KeyFrame::IsInImage */
            const float p0 = mp.pos[0] - s.Ow[0], p1 = mp.pos[1] - s.Ow[1], p2 = mp.pos[2] - s.Ow[2];
            const float dist = vslam_md::norm3(p0, p1, p2);
            if (dist < mp.min_distance || dist > mp.max_distance) continue;
            if (vslam_md::dot3_mat(p0, p1, p2, mp.normal) < 0.5 * (double)dist) continue;
            const int level = vslam_md::predict_level(mp.max_distance, dist, p->log_scale_factor, nlevels);
            const float radius = th * scale_factors[level];
            gated++;
            grid.query(uv.u, uv.v, radius, -1, -1, vIndices);
            if (vIndices.empty()) continue;
            const uint8_t* dMP = mp_desc + (size_t)iMP * 32;
            int bestDist = 256, bestIdx = -1;
            for (int idx : vIndices) {
                if (matched[idx]) continue;
                const int kpLevel = s.dev_kps[idx].octave;
                if (kpLevel < level - 1 || kpLevel > level) continue;
                const int d = rig_hamming(dMP, s.dev_desc + (size_t)idx * 32);
                if (d < bestDist) {
                    bestDist = d;
                    bestIdx = idx;
                }
            }
            if (bestDist <= thr) {
                match_kf[j][bestIdx] = iMP;
                matched[bestIdx] = 1;
                nm++;
            }
        }
        nmatches[j] = nm;
        if (n_gated) n_gated[j] = gated;
    }
    return VSLAM_OK;
}

/* FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (fmatcher.cpp:546-748) with F.Nleft != -1 as it is
 * written, sequential, for one keyframe: the statement vslam_search_by_bow_rig is tested against, and the shim's fallback
 * beyond the device limits (there are none here).  Descriptor rows and FeatureVector indices of either side run over
 * [0, n_left + n_right), left first; kf_kps is ONE array (mvKeys then mvKeysRight), the frame's keypoints come per camera.
 * The right branch is nested in `bestDist1 <= TH_LOW` and its ratio test is `|| true`; one histogram takes both sides. */
int vslamh_search_by_bow_rig(const vslam_kp* kf_kps, const uint8_t* kf_desc_left, int kf_n_left, const uint8_t* kf_desc_right,
                             int kf_n_right, const uint8_t* kf_flags, const int32_t* kf_fv_nodes, const int32_t* kf_fv_off,
                             const int32_t* kf_fv_feat, int n_kf_nodes, const vslam_kp* f_kps_left, const uint8_t* f_desc_left,
                             int n_left, const vslam_kp* f_kps_right, const uint8_t* f_desc_right, int n_right,
                             const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat, int n_f_nodes,
                             float nnratio, int check_orientation, int32_t* match_f, int* nmatches) {
    const int nKF = kf_n_left + kf_n_right, N = n_left + n_right;
    if (kf_n_left < 0 || kf_n_right < 0 || n_left < 0 || n_right < 0 || n_kf_nodes < 0 || n_f_nodes < 0 || !nmatches ||
        (nKF && (!kf_kps || !kf_flags)) || (kf_n_left && !kf_desc_left) || (kf_n_right && !kf_desc_right) ||
        (n_left && (!f_kps_left || !f_desc_left)) || (n_right && (!f_kps_right || !f_desc_right)) || (N && !match_f) ||
        (n_kf_nodes && (!kf_fv_nodes || !kf_fv_off || !kf_fv_feat)) || (n_f_nodes && (!f_fv_nodes || !f_fv_off || !f_fv_feat)))
        return VSLAM_ERR_INVALID;
    *nmatches = 0;
    for (int i = 0; i < N; i++) match_f[i] = -1;
    for (int side = 0; side < 2; side++) {
        const int32_t *off = side ? f_fv_off : kf_fv_off, *feat = side ? f_fv_feat : kf_fv_feat;
        const int nn = side ? n_f_nodes : n_kf_nodes, n = side ? N : nKF;
        if (nn && off[0] != 0) return VSLAM_ERR_INVALID;
        for (int j = 0; j < nn; j++) {
            if (off[j + 1] < off[j]) return VSLAM_ERR_INVALID;
            for (int a = off[j]; a < off[j + 1]; a++)
                if (feat[a] < 0 || feat[a] >= n) return VSLAM_ERR_INVALID;
        }
    }
    const int TH_LOW = 50, L = VSLAM_HISTO_LENGTH;
    std::vector<int> rotHist[VSLAM_HISTO_LENGTH];
    int nm = 0;
    int KFit = 0, Fit = 0;
    while (KFit != n_kf_nodes && Fit != n_f_nodes) {
        if (kf_fv_nodes[KFit] == f_fv_nodes[Fit]) {
            for (int a = kf_fv_off[KFit]; a < kf_fv_off[KFit + 1]; a++) {
                const int realIdxKF = kf_fv_feat[a];
                if (!kf_flags[realIdxKF]) continue; /* !pMP || pMP->isBad() */
                const uint8_t* dKF = realIdxKF < kf_n_left ? kf_desc_left + (size_t)realIdxKF * 32
                                                           : kf_desc_right + (size_t)(realIdxKF - kf_n_left) * 32;
                int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
                int bestDist1R = 256, bestIdxFR = -1;
                for (int b = f_fv_off[Fit]; b < f_fv_off[Fit + 1]; b++) {
                    const int realIdxF = f_fv_feat[b];
                    if (match_f[realIdxF] >= 0) continue;
                    const uint8_t* dF = realIdxF < n_left ? f_desc_left + (size_t)realIdxF * 32
                                                          : f_desc_right + (size_t)(realIdxF - n_left) * 32;
                    const int dist = rig_hamming(dKF, dF);
                    if (realIdxF < n_left && dist < bestDist1) {
                        bestDist2 = bestDist1;
                        bestDist1 = dist;
                        bestIdxF = realIdxF;
                    } else if (realIdxF < n_left && dist < bestDist2) {
                        bestDist2 = dist;
                    }
                    if (realIdxF >= n_left && dist < bestDist1R) {
                        bestDist1R = dist;
                        bestIdxFR = realIdxF;
                    }
                }
                if (bestDist1 <= TH_LOW) {
                    const float angKF = kf_kps[realIdxKF].angle;
                    if ((float)bestDist1 < nnratio * (float)bestDist2) {
                        match_f[bestIdxF] = realIdxKF;
                        if (check_orientation) rotHist[vslam_md::rot_bin(angKF, f_kps_left[bestIdxF].angle, L)].push_back(bestIdxF);
                        nm++;
                    }
                    if (bestDist1R <= TH_LOW) { /* `|| true`, :682 */
                        match_f[bestIdxFR] = realIdxKF;
                        if (check_orientation)
                            rotHist[vslam_md::rot_bin(angKF, f_kps_right[bestIdxFR - n_left].angle, L)].push_back(bestIdxFR);
                        nm++;
                    }
                }
            }
            KFit++;
            Fit++;
        } else if (kf_fv_nodes[KFit] < f_fv_nodes[Fit]) {
            KFit = (int)(std::lower_bound(kf_fv_nodes, kf_fv_nodes + n_kf_nodes, f_fv_nodes[Fit]) - kf_fv_nodes);
        } else {
            Fit = (int)(std::lower_bound(f_fv_nodes, f_fv_nodes + n_f_nodes, kf_fv_nodes[KFit]) - f_fv_nodes);
        }
    }
    if (check_orientation) {
        int histo[VSLAM_HISTO_LENGTH];
        for (int b = 0; b < L; b++) histo[b] = (int)rotHist[b].size();
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(histo, L);
        for (int b = 0; b < L; b++)
            if (!vslam_md::keeps_bin(mx, b))
                for (int s : rotHist[b]) {
                    match_f[s] = -1;
                    nm--;
                }
    }
    *nmatches = nm;
    return VSLAM_OK;
}

/* vslam_two_view_score on the host, every pointer of the job a HOST pointer (the placement fields are not read): the pair
 * list, CheckHomography / CheckFundamental for every hypothesis by the shared vslam_two_view.h code, the selection.  Same
 * limits, error codes and results as the device entry (include/vslam_fe.h).  CPU tests and the stand-alone demo; the
 * product runs k_tv_pairs / k_tv_score / k_tv_select. */
int vslamh_two_view_score(const vslam_two_view_job* job, vslam_two_view_result* result) {
    if (!job || !result) return VSLAM_ERR_INVALID;
    const vslam_two_view_job& q = *job;
    if (q.n1 < 0 || q.n1 > 65536 || q.n2 < 0 || q.nH < 0 || q.nH > VSLAM_TWO_VIEW_MAX_HYP || q.nF < 0 ||
        q.nF > VSLAM_TWO_VIEW_MAX_HYP || (q.n1 && (!q.kps1 || !q.matches12)) || (q.n1 && q.n2 && !q.kps2) ||
        (q.nH && (!q.H21 || !q.H12)) || (q.nF && !q.F21) || !std::isfinite(q.sigma) || q.sigma == 0.0f)
        return VSLAM_ERR_INVALID;
    vslam_two_view_result& R = *result;
    const int cap = std::min(q.n1, VSLAM_TWO_VIEW_MAX_PAIRS);
    std::vector<float> pts;
    std::vector<int32_t> pairs;
    int n = 0;
    bool err = false;
    for (int i = 0; i < q.n1; i++) { /* motion_estimation.cpp:2020-2029 */
        const int32_t m = q.matches12[i];
        if (m >= q.n2) err = true;
        if (m < 0 || m >= q.n2) continue;
        if (n < cap) {
            pairs.insert(pairs.end(), {i, m});
            pts.insert(pts.end(), {q.kps1[i].x, q.kps1[i].y, q.kps2[m].x, q.kps2[m].y});
        }
        n++;
    }
    const int used = (err || n > cap) ? 0 : n;
    const float inv = vslam_tv::inv_sigma_square(q.sigma);
    R.n_pairs = n;
    if (R.pairs && !pairs.empty()) memcpy(R.pairs, pairs.data(), pairs.size() * 4);
    std::vector<uint8_t> cur((size_t)used);
    for (int model = 0; model < 2; model++) {
        const int nhyp = model ? q.nF : q.nH;
        float* scores = model ? R.scores_f : R.scores_h;
        uint8_t* mask = model ? R.inliers_f : R.inliers_h;
        vslam_tv::Best best = vslam_tv::best_none();
        if (mask && used) memset(mask, 0, (size_t)used);
        for (int it = 0; it < nhyp; it++) {
            const vslam_tv::Mat3 A = vslam_tv::load_mat3((model ? q.F21 : q.H21) + (size_t)it * 9);
            const vslam_tv::Mat3 B = model ? A : vslam_tv::load_mat3(q.H12 + (size_t)it * 9);
            float score = 0.0f;
            for (int p = 0; p < used; p++) {
                const float* x = &pts[4 * (size_t)p];
                const vslam_tv::Terms t = model ? vslam_tv::check_f(A, x[0], x[1], x[2], x[3], inv)
                                                : vslam_tv::check_h(A, B, x[0], x[1], x[2], x[3], inv);
                score = vslam_tv::fadd(score, t.t1);
                score = vslam_tv::fadd(score, t.t2);
                cur[p] = t.in ? 1 : 0;
            }
            score = vslam_tv::report_score(score);
            if (scores) scores[it] = score;
            const vslam_tv::Best was = best;
            best = vslam_tv::best_take(best, score, it);
            if (best.index != was.index && mask && used) memcpy(mask, cur.data(), (size_t)used);
        }
        (model ? R.best_f : R.best_h) = best.index;
        (model ? R.score_f : R.score_h) = best.index >= 0 ? best.score : 0.0f;
    }
    return err ? VSLAM_ERR_INVALID : n > cap ? VSLAM_ERR_UNSUPPORTED : VSLAM_OK;
}

uint64_t vslamh_layout(uint64_t align, const uint64_t* sizes, int n, uint64_t* off) {
    std::vector<size_t> s(sizes, sizes + n), o(n);
    const size_t total = vslam::layout_parts((size_t)align, s.data(), n, o.data());
    for (int i = 0; i < n; i++) off[i] = o[i];
    return total;
}

/* quadtree path tables of k_octree_v4 against the literal halvings: returns the number of (x, y) whose table path differs */
int vslamh_oct_lut_check(int W, int H, int D) {
    std::vector<uint32_t> xs, ys;
    vslam::build_oct_lut(W, H, D, xs, ys);
    int bad = 0;
    for (int y = 0; y <= H; y++)
        for (int x = 0; x <= W; x++) bad += (xs[x] | ys[y]) != vslam::oct_key_path(x, y, W, H, D);
    return bad;
}
unsigned vslamh_oct_key_path(int x, int y, int W, int H, int depth) { return vslam::oct_key_path(x, y, W, H, depth); }

int vslamh_keypoint_capacity(const int* quota, const int* lw, const int* lh, int nlevels, int nfeatures) {
    return vslam::keypoint_capacity(quota, lw, lh, nlevels, nfeatures);
}

/* plan_octree with node arrays of node_per * maxNodes + node_fixed bytes.  ctx6 = maxNodes, selStride, fineLdsOff,
 * fineLdsBytes, fits, number of (x, y) of all levels whose table path differs from oct_key_path at the level's depth;
 * lvl4 rows = nIni, selOff, fineD, lutW */
int vslamh_oct_plan(const int* quota, const int* lw, const int* lh, const int* cell_first, int nlevels, int forced_depth,
                    int budget, int node_per, int node_fixed, int32_t* ctx6, int32_t* lvl4) {
    vslam::OctPlan P;
    vslam::plan_octree(quota, lw, lh, cell_first, nlevels, forced_depth, (size_t)budget,
                       [=](int n) { return (size_t)n * node_per + node_fixed; }, P);
    int bad = 0;
    for (int l = 0; l < nlevels; l++) {
        const int W = P.lutW[l] - 1, H = P.H[l];
        const uint32_t *xs = P.lut.data() + P.lutOff[l], *ys = xs + P.lutW[l];
        for (int y = 0; y <= H; y++)
            for (int x = 0; x <= W; x++) bad += (xs[x] | ys[y]) != vslam::oct_key_path(x, y, W, H, P.fineD[l]);
        const int32_t o[4] = {P.nIni[l], P.selOff[l], P.fineD[l], P.lutW[l]};
        memcpy(lvl4 + 4 * l, o, sizeof(o));
    }
    const int32_t c[6] = {P.maxNodes, P.selStride, P.fineLdsOff, P.fineLdsBytes, P.fits, bad};
    memcpy(ctx6, c, sizeof(c));
    return 0;
}

/* pack_bands over the bands of a cell list (rows as vslamh_cells writes them, all levels): words4 rows = BandWords, classes =
 * 272 bytes per class; info5 = classes, max_wh, max_iw, max_cells, ok.  Returns the bands, -1 if a buffer is too small. */
int vslamh_band_tables(const uint16_t* cells5, int ncells, int nlevels, int max_cells, int max_width, uint32_t* words4,
                       int cap_bands, uint8_t* classes, int cap_class_bytes, int32_t* info5) {
    static_assert(sizeof(vslam::HostCell) == 10 && sizeof(vslam::BandWords) == 16, "rows of five u16 / four u32");
    const vslam::HostCell* c = (const vslam::HostCell*)cells5;
    std::vector<vslam::HostBand> b;
    vslam::build_bands(std::vector<vslam::HostCell>(c, c + ncells), max_cells, max_width, b);
    vslam::BandTables T;
    vslam::pack_bands(b, nlevels, T);
    if ((int)b.size() > cap_bands || (int)T.classes.size() > cap_class_bytes) return -1;
    memcpy(words4, T.bands.data(), T.bands.size() * sizeof(vslam::BandWords));
    memcpy(classes, T.classes.data(), T.classes.size());
    const int32_t o[5] = {(int32_t)(T.classes.size() / 272), T.max_wh, T.max_iw, T.max_cells, T.ok};
    memcpy(info5, o, sizeof(o));
    return (int)b.size();
}

} /* extern "C" */

/* ------------------------------------------------------------------ ComputeBoW, host half
 * DBoW3::Vocabulary::transform (Vocabulary.cpp:754-826) after the per-feature tree walk: BowVector::addWeight /
 * addIfNotExist in feature order (std::map, double), the "divide by the number of words" step when the scoring
 * object does not normalise, BowVector::normalize (BowVector.cpp), FeatureVector::addFeature. */
extern "C" int vslam_bow_assemble(int weighting, int norm, const int32_t* word_id, const double* weight,
                                  const int32_t* node_id, int n, int32_t* bow_ids, double* bow_vals, int* n_bow,
                                  int32_t* fv_nodes, int32_t* fv_off, int32_t* fv_feat, int* n_fv) {
    if (n < 0 || (n && (!word_id || !weight || !node_id || !bow_ids || !bow_vals || !fv_nodes || !fv_off || !fv_feat)) ||
        !n_bow || !n_fv || weighting < 0 || weighting > 3 || norm < 0 || norm > 2)
        return -1;
    /* std::map semantics without the tree: a STABLE sort of the kept feature indices by word id (by node id) keeps
     * the feature order inside each key, so every word's weights are summed in exactly the order addWeight saw them */
    std::vector<int32_t> kept;
    kept.reserve(n);
    for (int i = 0; i < n; i++)
        if (weight[i] > 0) kept.push_back(i); /* not stopped */
    const bool tf = weighting == 0 || weighting == 1; /* TF_IDF, TF */
    std::vector<int32_t> byWord(kept);
    std::stable_sort(byWord.begin(), byWord.end(), [&](int32_t a, int32_t b) { return word_id[a] < word_id[b]; });
    int k = 0;
    for (size_t p = 0; p < byWord.size();) {
        const int32_t w = word_id[byWord[p]];
        double v = 0.0;
        bool first = true;
        size_t q = p;
        for (; q < byWord.size() && word_id[byWord[q]] == w; q++) {
            if (tf) v = first ? weight[byWord[q]] : v + weight[byWord[q]]; /* insert, then += */
            else if (first) v = weight[byWord[q]];                       /* addIfNotExist */
            first = false;
        }
        bow_ids[k] = w;
        bow_vals[k++] = v;
        p = q;
    }
    if (tf && k > 0 && norm == 0) {
        const double nd = (double)k;
        for (int i = 0; i < k; i++) bow_vals[i] /= nd;
    }
    if (norm) {
        double nv = 0.0;
        if (norm == 1) for (int i = 0; i < k; i++) nv += std::fabs(bow_vals[i]);
        else {
            for (int i = 0; i < k; i++) nv += bow_vals[i] * bow_vals[i];
            nv = std::sqrt(nv);
        }
        if (nv > 0.0) for (int i = 0; i < k; i++) bow_vals[i] /= nv;
    }
    *n_bow = k;
    std::vector<int32_t> byNode(kept);
    std::stable_sort(byNode.begin(), byNode.end(), [&](int32_t a, int32_t b) { return node_id[a] < node_id[b]; });
    int f = 0, off = 0;
    for (size_t p = 0; p < byNode.size();) {
        const int32_t nd = node_id[byNode[p]];
        fv_nodes[f] = nd;
        fv_off[f++] = off;
        for (; p < byNode.size() && node_id[byNode[p]] == nd; p++) fv_feat[off++] = byNode[p];
    }
    fv_off[f] = off;
    *n_fv = f;
    return 0;
}

/* ------------------------------------------------------------------ KeyFrameDatabase, selection stage
 * DetectRelocalizationCandidates (keyframedatabase.cpp:707-811) and DetectNBestCandidates (:579-705) from the hit list
 * on: the hits are lKFsSharingWords in the reference's order (vslam_kfdb_query_wait), words / si what the walk and
 * mpVoc->score leave in the KeyFrames, score_io the mRelocScore / mPlaceRecognitionScore members (read stale for
 * hits that are not scored by this query, written for those that are). */
#include <unordered_map>
#include <unordered_set>

namespace {
struct KfdbScored {
    float score;
    int hit;
};

/* :732-789 (:615-675): maxCommonWords, minCommonWords, the scores, the covisibility accumulation.  `listed[i]` == 0:
 * hit i never entered lKFsSharingWords (a connected keyframe, :600).  Returns lAccScoreAndMatch and bestAccScore. */
std::vector<KfdbScored> kfdb_accumulate(const int64_t* hit_kf, const int32_t* hit_words, const float* hit_si, int n_hits,
                                        const uint8_t* listed, float* score_io, vslam_kfdb_neighbours_fn neighbours_fn,
                                        void* user, float* bestAccScore) {
    std::vector<KfdbScored> acc;
    *bestAccScore = 0;
    int maxCommonWords = 0;
    for (int i = 0; i < n_hits; i++)
        if (listed[i] && hit_words[i] > maxCommonWords) maxCommonWords = hit_words[i];
    const int minCommonWords = (int)(maxCommonWords * 0.8f);
    std::vector<KfdbScored> scored; /* lScoreAndMatch */
    for (int i = 0; i < n_hits; i++)
        if (listed[i] && hit_words[i] > minCommonWords) {
            score_io[i] = hit_si[i];
            scored.push_back({hit_si[i], i});
        }
    if (scored.empty()) return acc;
    std::unordered_map<int64_t, int> byId; /* mn*Query == this query's id */
    for (int i = 0; i < n_hits; i++)
        if (listed[i]) byId.emplace(hit_kf[i], i);
    for (const KfdbScored& sc : scored) {
        int64_t neigh[10];
        int nn = neighbours_fn ? neighbours_fn(user, hit_kf[sc.hit], neigh) : 0;
        if (nn > 10) nn = 10;
        float bestScore = sc.score, accScore = bestScore;
        int best = sc.hit;
        for (int k = 0; k < nn; k++) {
            auto it = byId.find(neigh[k]);
            if (it == byId.end()) continue;
            const float s2 = score_io[it->second];
            accScore += s2;
            if (s2 > bestScore) {
                best = it->second;
                bestScore = s2;
            }
        }
        acc.push_back({accScore, best});
        if (accScore > *bestAccScore) *bestAccScore = accScore;
    }
    return acc;
}

bool kfdb_hits_ok(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words, const float* hit_si, int n_hits,
                  const float* score_io) {
    return n_hits >= 0 && (n_hits == 0 || (hit_kf && hit_map && hit_words && hit_si && score_io));
}
} /* namespace */

extern "C" int vslam_kfdb_select_relocalization(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words,
                                                const float* hit_si, int n_hits, float* score_io, int32_t map_id,
                                                vslam_kfdb_neighbours_fn neighbours_fn, void* user, int64_t* out_kf,
                                                int cap, int* n_out) {
    if (!kfdb_hits_ok(hit_kf, hit_map, hit_words, hit_si, n_hits, score_io) || !n_out || cap < 0 || (cap && !out_kf))
        return -1;
    *n_out = 0;
    if (n_hits == 0) return 0; /* :729 */
    const std::vector<uint8_t> listed((size_t)n_hits, 1);
    float bestAccScore;
    const std::vector<KfdbScored> acc =
        kfdb_accumulate(hit_kf, hit_words, hit_si, n_hits, listed.data(), score_io, neighbours_fn, user, &bestAccScore);
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::unordered_set<int> added; /* spAlreadyAddedKF */
    std::vector<int64_t> out;
    for (const KfdbScored& a : acc)
        if (a.score > minScoreToRetain) {
            if (hit_map[a.hit] != map_id) continue;
            if (added.insert(a.hit).second) out.push_back(hit_kf[a.hit]);
        }
    *n_out = (int)out.size();
    if ((int)out.size() > cap) return -4; /* VSLAM_ERR_CAPACITY; *n_out says how many there are */
    for (size_t i = 0; i < out.size(); i++) out_kf[i] = out[i];
    return 0;
}

extern "C" int vslam_kfdb_select_nbest(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words,
                                       const float* hit_si, int n_hits, float* score_io, int32_t query_map_id,
                                       const int64_t* connected_ids, int n_connected, int n_candidates,
                                       const int32_t* bad_maps, int n_bad_maps, vslam_kfdb_neighbours_fn neighbours_fn,
                                       void* user, int64_t* loop_kf, int* n_loop, int64_t* merge_kf, int* n_merge) {
    if (!kfdb_hits_ok(hit_kf, hit_map, hit_words, hit_si, n_hits, score_io) || n_connected < 0 ||
        (n_connected && !connected_ids) || n_bad_maps < 0 || (n_bad_maps && !bad_maps) || n_candidates < 0 || !n_loop ||
        !n_merge || (n_candidates && (!loop_kf || !merge_kf)))
        return -1;
    *n_loop = *n_merge = 0;
    const std::unordered_set<int64_t> connected(connected_ids, connected_ids + n_connected); /* spConnectedKF */
    std::vector<uint8_t> listed((size_t)n_hits);
    bool any = false;
    for (int i = 0; i < n_hits; i++) any |= (listed[i] = !connected.count(hit_kf[i])) != 0; /* :600 */
    if (!any) return 0; /* :612 */
    float bestAccScore;
    std::vector<KfdbScored> acc =
        kfdb_accumulate(hit_kf, hit_words, hit_si, n_hits, listed.data(), score_io, neighbours_fn, user, &bestAccScore);
    /* list::sort(compFirst) is a stable merge sort, descending */
    std::stable_sort(acc.begin(), acc.end(), [](const KfdbScored& a, const KfdbScored& b) { return a.score > b.score; });
    std::unordered_set<int> added; /* spAlreadyAddedKF */
    for (size_t i = 0; i < acc.size() && (*n_loop < n_candidates || *n_merge < n_candidates); i++) { /* :684-704 */
        const int h = acc[i].hit;
        if (added.count(h)) continue;
        const int32_t map = hit_map[h];
        if (query_map_id == map && *n_loop < n_candidates) loop_kf[(*n_loop)++] = hit_kf[h];
        else if (query_map_id != map && *n_merge < n_candidates &&
                 std::find(bad_maps, bad_maps + n_bad_maps, map) == bad_maps + n_bad_maps)
            merge_kf[(*n_merge)++] = hit_kf[h];
        added.insert(h);
    }
    return 0;
}

/* ------------------------------------------------------------------------------------------------------------------
 * vilib::FeatureTrackerGPU's bookkeeping (include/vslam_featuretracker.h): steps 02 and 03 of track() and what they
 * call, around the two kernels of vslam_featuretracker.hip.  feature_tracker_gpu.cpp:137-267,319-352,404-411,496-524;
 * feature_tracker_base.cpp:61-171.
 * ------------------------------------------------------------------------------------------------------------------ */
#include "../../include/vslam_featuretracker.h"

struct vslam_ftbook {
    vslam_ft_params p;
    int n_cols = 0, n_rows = 0, cw = 0, ch = 0, cells = 0, max_ftr = 0;
    int next_id = 0, tracked = 0, detected = 0;
    struct Track {
        vslam_ft_track_info i;
        int first_level;
        float first_score;
    };
    std::vector<Track> tracks;
    std::vector<int> avail; /* available_indices_: decreasing, taken from the back */
    std::vector<vslam_ft_feature> feats;
    void add_feature(const Track& t) { feats.push_back(vslam_ft_feature{t.i.cur_pos[0], t.i.cur_pos[1], t.first_score, t.first_level, t.i.track_id}); }
};

extern "C" int vslam_ftbook_create(const vslam_ft_params* p, int n_cols, int n_rows, int cell_w, int cell_h, vslam_ftbook** out) {
    if (!p || !out || n_cols < 1 || n_rows < 1 || cell_w < 1 || cell_h < 1 || p->use_best_n_features < -1 ||
        p->min_tracks_to_detect_new_features < 0)
        return -1;
    *out = nullptr;
    const long long cells = (long long)n_cols * n_rows;
    /* feature_tracker_gpu.cpp:404-411 */
    const long long max_ftr = ((long long)p->min_tracks_to_detect_new_features - 1) + ((p->use_best_n_features == -1 ? cells : p->use_best_n_features) - 1);
    if (max_ftr < 1 || max_ftr > (1 << 20)) return -1;
    vslam_ftbook* b = new vslam_ftbook();
    b->p = *p;
    b->n_cols = n_cols;
    b->n_rows = n_rows;
    b->cw = cell_w;
    b->ch = cell_h;
    b->cells = (int)cells;
    b->max_ftr = (int)max_ftr;
    for (int i = 0; i < b->max_ftr; i++) b->avail.push_back(b->max_ftr - i - 1); /* initBufferIds */
    *out = b;
    return 0;
}

extern "C" void vslam_ftbook_destroy(vslam_ftbook* b) { delete b; }
extern "C" int vslam_ftbook_capacity(const vslam_ftbook* b) { return b ? b->max_ftr : -1; }

extern "C" int vslam_ftbook_results(vslam_ftbook* b, const float* res, int n) {
    if (!b || n != (int)b->tracks.size() || (n && !res)) return -1;
    b->feats.clear();
    b->tracked = 0;
    std::vector<vslam_ftbook::Track> keep; /* removeTracks: the survivors in their order */
    keep.reserve(b->tracks.size());
    for (int i = 0; i < n; i++) {
        vslam_ftbook::Track& t = b->tracks[i];
        const float x = res[4 * i];
        if (std::isnan(x)) {
            b->avail.push_back(t.i.buffer_id);
            continue;
        }
        t.i.life++;
        t.i.cur_pos[0] = x;
        t.i.cur_pos[1] = res[4 * i + 1];
        t.i.cur_disparity = res[4 * i + 2];
        b->tracked++;
        b->add_feature(t);
        keep.push_back(t);
    }
    b->tracks.swap(keep);
    b->detected = 0;
    return 0;
}

extern "C" int vslam_ftbook_need_detect(const vslam_ftbook* b) { return b ? (b->tracked < b->p.min_tracks_to_detect_new_features ? 1 : 0) : -1; }

extern "C" int vslam_ftbook_detect(vslam_ftbook* b, const float* pos, const float* score, const int32_t* level, int* n_detected) {
    if (!b || !pos || !score || !level) return -1;
    b->detected = 0;
    std::vector<uint8_t> occ((size_t)b->cells, 0); /* OccupancyGrid2D::reset */
    if (b->p.reset_before_detection) {
        b->tracked = 0;
        for (const vslam_ftbook::Track& t : b->tracks) b->avail.push_back(t.i.buffer_id);
        b->tracks.clear();
        b->feats.clear();
    } else {
        for (const vslam_ft_feature& f : b->feats) { /* setOccupied(int x, int y): the position truncated */
            const double fx = (double)f.x, fy = (double)f.y;
            if (!(fx > -1.0 && fy > -1.0 && fx < (double)b->n_cols * b->cw && fy < (double)b->n_rows * b->ch)) continue; /* the reference asserts */
            const int x = (int)fx, y = (int)fy;
            occ[(size_t)(y / b->ch) * b->n_cols + x / b->cw] = 1;
        }
    }
    std::vector<int> order((size_t)b->cells);
    for (int i = 0; i < b->cells; i++) order[i] = i;
    int limit = b->cells;
    if (b->p.use_best_n_features != -1) { /* :242-247; the reference's std::sort leaves ties open: the lower cell first */
        std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return score[a] > score[c]; });
        limit = std::max(0, b->p.use_best_n_features - b->tracked);
    }
    for (int k = 0; k < b->cells && b->detected < limit && !b->avail.empty(); k++) {
        const int c = order[k];
        if (occ[c] || !(score[c] > 0.0f)) continue;
        vslam_ftbook::Track t;
        memset(&t, 0, sizeof(t));
        t.i.first_pos[0] = t.i.cur_pos[0] = pos[2 * c];
        t.i.first_pos[1] = t.i.cur_pos[1] = pos[2 * c + 1];
        t.i.track_id = b->next_id++;
        t.i.buffer_id = b->avail.back();
        b->avail.pop_back();
        t.first_level = level[c];
        t.first_score = score[c];
        b->tracks.push_back(t);
        b->add_feature(t);
        b->detected++;
    }
    if (n_detected) *n_detected = b->detected;
    return 0;
}

extern "C" int vslam_ftbook_update_count(const vslam_ftbook* b) {
    return b ? (b->p.klt_template_is_first_observation ? b->detected : b->detected + b->tracked) : -1;
}

extern "C" int vslam_ftbook_features(const vslam_ftbook* b, vslam_ft_feature* out, int cap, int* n) {
    if (!b || cap < 0 || (cap && !out)) return -1;
    if (n) *n = (int)b->feats.size();
    for (int i = 0; i < cap && i < (int)b->feats.size(); i++) out[i] = b->feats[i];
    return 0;
}

extern "C" int vslam_ftbook_tracks(const vslam_ftbook* b, vslam_ft_track_info* out, int cap, int* n) {
    if (!b || cap < 0 || (cap && !out)) return -1;
    if (n) *n = (int)b->tracks.size();
    for (int i = 0; i < cap && i < (int)b->tracks.size(); i++) out[i] = b->tracks[i].i;
    return 0;
}

extern "C" int vslam_ftbook_disparity(const vslam_ftbook* b, double pivot_ratio, double* out) {
    if (!b || !out || !(pivot_ratio >= 0.0)) return -1;
    std::vector<float> d; /* tracks with life >= 1; new tracks sit at the end of the list */
    for (const vslam_ftbook::Track& t : b->tracks) {
        if (t.i.life <= 0) break;
        d.push_back(t.i.cur_disparity);
    }
    *out = 0.0;
    if (d.empty()) return 0;
    const size_t pivot = std::min((size_t)(pivot_ratio * (double)d.size()), d.size() - 1);
    std::nth_element(d.begin(), d.begin() + pivot, d.end());
    *out = (double)d[pivot];
    return 0;
}

extern "C" int vslam_ftbook_reset(vslam_ftbook* b) {
    if (!b) return -1;
    for (const vslam_ftbook::Track& t : b->tracks) b->avail.push_back(t.i.buffer_id);
    b->tracks.clear();
    b->tracked = b->detected = 0;
    return 0;
}

extern "C" int vslam_ftbook_set_best_n(vslam_ftbook* b, int n) {
    if (!b || n < -1) return -1;
    b->p.use_best_n_features = n;
    return 0;
}

extern "C" int vslam_ftbook_set_min_tracks(vslam_ftbook* b, int n) {
    if (!b || n < 0) return -1;
    b->p.min_tracks_to_detect_new_features = n;
    return 0;
}

/* Point::getNewId is one counter for every camera of a FrameBundle: a tracker over several books reads it from one book
 * after step 03 and hands it to the next before */
extern "C" int vslam_ftbook_next_id(const vslam_ftbook* b) { return b ? b->next_id : -1; }
extern "C" int vslam_ftbook_set_next_id(vslam_ftbook* b, int id) {
    if (!b || id < 0) return -1;
    b->next_id = id;
    return 0;
}
