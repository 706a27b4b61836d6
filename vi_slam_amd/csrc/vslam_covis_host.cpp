/* vslam_covis_host.cpp -- the host shadow of the observation graph (vslam_covis.h): the bookkeeping behind the
 * vslam_covis_* mutators, and the queries answered from the shadow (vslamh_covis_*: the CPU tests and the demo; not a
 * fallback of the device form).  Plain C++, compiled into libvslam_fe.so and libvslam_host.so.
 *
 * Cost of a mutation: O(records of the point) on the host (a point has a handful), and 256-byte chunks marked dirty:
 * one of ptab, and for an observation one of the pool (a moved segment: its chunks).  A keyframe mutation marks the two
 * keyframe tables, which go up whole (20 bytes per slot) after the ranks by order_key were recomputed. */
#include "vslam_covis.h"

#include <algorithm>
#include <cstring>

void CovisArray::take(size_t used, std::vector<CovisRange>& out) {
    if (all) {
        if (used) out.push_back({0u, (uint32_t)used});
    } else {
        std::sort(dirty_list.begin(), dirty_list.end());
        for (size_t i = 0; i < dirty_list.size(); i++) {
            const size_t lo = (size_t)dirty_list[i] * COVIS_CHUNK_WORDS;
            if (lo >= used) continue;
            const size_t hi = std::min(lo + COVIS_CHUNK_WORDS, used);
            if (!out.empty() && (size_t)out.back().off + out.back().n == lo)
                out.back().n += (uint32_t)(hi - lo);
            else
                out.push_back({(uint32_t)lo, (uint32_t)(hi - lo)});
        }
    }
    for (uint32_t c : dirty_list) dirty[c] = 0;
    dirty_list.clear();
    all = false;
}

CovisStore::CovisStore(size_t initial_entries) {
    cap = initial_entries ? initial_entries : COVIS_DEFAULT_ENTRIES;
    if (cap < COVIS_FIRST_SEGMENT) cap = COVIS_FIRST_SEGMENT;
    pool.w.assign(cap * 2, 0);
    extra.resize(cap);
}

/* ------------------------------------------------------------------ keyframes */
int CovisStore::add_keyframe(int64_t kf, int32_t map, uint64_t key) {
    if (kf_slot.count(kf)) return fail("covis add_keyframe: the keyframe is in the mirror already");
    if (key_slot.count(key)) return fail("covis add_keyframe: order_key is in use by a live keyframe");
    int32_t s;
    if (!kf_free.empty()) {
        s = kf_free.back();
        kf_free.pop_back();
    } else {
        s = (int32_t)kf_id.size();
        kf_id.push_back(0);
        kf_key.push_back(0);
        kf_refs.push_back(0);
        ktab.resize(ktab.size() + 4, 0);
    }
    kf_id[s] = kf;
    kf_key[s] = key;
    kf_refs[s] = 0;
    ktab[(size_t)s * 4 + 0] = 0;
    ktab[(size_t)s * 4 + 1] = map;
    ktab[(size_t)s * 4 + 2] = COVIS_ALIVE;
    kf_slot[kf] = s;
    key_slot[key] = s;
    ranks_stale = k_upload = true;
    return VSLAM_OK;
}

int CovisStore::add_keyframes(int n, const int64_t* kf, const int32_t* map, const uint64_t* key) {
    if (n < 0 || (n && (!kf || !map || !key))) return fail("covis add_keyframes: invalid arguments");
    std::unordered_map<int64_t, int> ids;
    std::unordered_map<uint64_t, int> keys;
    for (int i = 0; i < n; i++) { /* all or none */
        if (kf_slot.count(kf[i]) || !ids.emplace(kf[i], i).second)
            return fail("covis add_keyframes: a keyframe is in the mirror already or listed twice");
        if (key_slot.count(key[i]) || !keys.emplace(key[i], i).second)
            return fail("covis add_keyframes: an order_key is in use or listed twice");
    }
    for (int i = 0; i < n; i++) add_keyframe(kf[i], map[i], key[i]);
    return VSLAM_OK;
}

int CovisStore::set_keyframe_bad(int64_t kf) {
    auto it = kf_slot.find(kf);
    if (it == kf_slot.end()) return fail("covis set_keyframe_bad: unknown keyframe");
    ktab[(size_t)it->second * 4 + 2] |= COVIS_BAD;
    k_upload = true;
    return VSLAM_OK;
}

int CovisStore::set_keyframe_map(int64_t kf, int32_t map) {
    auto it = kf_slot.find(kf);
    if (it == kf_slot.end()) return fail("covis set_keyframe_map: unknown keyframe");
    ktab[(size_t)it->second * 4 + 1] = map;
    k_upload = true;
    return VSLAM_OK;
}

int CovisStore::erase_keyframe(int64_t kf) {
    auto it = kf_slot.find(kf);
    if (it == kf_slot.end()) return fail("covis erase_keyframe: unknown keyframe");
    const int32_t s = it->second;
    if (kf_refs[s]) return fail("covis erase_keyframe: a MapPoint still observes the keyframe");
    ktab[(size_t)s * 4 + 2] = 0;
    key_slot.erase(kf_key[s]);
    kf_slot.erase(it);
    kf_free.push_back(s);
    ranks_stale = k_upload = true;
    return VSLAM_OK;
}

void CovisStore::refresh_ranks() {
    if (!ranks_stale) return;
    korder.clear();
    for (size_t s = 0; s < kf_id.size(); s++)
        if (ktab[s * 4 + 2] & COVIS_ALIVE) korder.push_back((int32_t)s);
    std::sort(korder.begin(), korder.end(), [&](int32_t a, int32_t b) { return kf_key[a] < kf_key[b]; });
    for (size_t r = 0; r < korder.size(); r++) ktab[(size_t)korder[r] * 4 + 0] = (int32_t)r;
    ranks_stale = false;
    k_upload = true;
}

/* ------------------------------------------------------------------ points */
int CovisStore::add_point(int64_t mp) {
    if (mp < 0) return fail("covis add_point: ids are not negative");
    if (mp_slot.count(mp)) return fail("covis add_point: the MapPoint is in the mirror already");
    int32_t p;
    if (!mp_free.empty()) {
        p = mp_free.back();
        mp_free.pop_back();
    } else {
        p = (int32_t)mp_id.size();
        mp_id.push_back(0);
        seg_cap.push_back(0);
        ptab.w.resize(ptab.w.size() + 4, 0);
    }
    mp_id[p] = mp;
    seg_cap[p] = 0;
    set_ptab(p, 0, 0);
    set_ptab(p, 1, 0);
    set_ptab(p, 2, 0);
    set_ptab(p, 3, COVIS_ALIVE);
    mp_slot[mp] = p;
    return VSLAM_OK;
}

/* every record of the point leaves: the keyframes' reference counts follow */
void CovisStore::drop_records(int32_t p) {
    const size_t off = (uint32_t)ptab.w[(size_t)p * 4], len = (size_t)ptab.w[(size_t)p * 4 + 1];
    for (size_t i = 0; i < len; i++) kf_refs[pool.w[(off + i) * 2]]--;
    n_records -= len;
    set_ptab(p, 1, 0);
}

void CovisStore::drop_segment(int32_t p) {
    dead += seg_cap[p];
    seg_cap[p] = 0;
    set_ptab(p, 0, 0);
}

/* room for one more record of point p; returns its place in the pool */
int CovisStore::reserve_record(int32_t p) {
    const size_t off = (uint32_t)ptab.w[(size_t)p * 4], len = (size_t)ptab.w[(size_t)p * 4 + 1];
    const size_t have = seg_cap[p];
    if (len < have) return (int)(off + len);
    const size_t need = have ? have * 2 : COVIS_FIRST_SEGMENT;
    if (used + need > cap) {
        while (used + need > cap) cap *= 2;
        pool.w.resize(cap * 2, 0);
        extra.resize(cap);
        pool.all = true; /* the device array is allocated anew */
        n_grow++;
    }
    const size_t to = used;
    used += need;
    if (len) {
        memcpy(&pool.w[to * 2], &pool.w[off * 2], len * 8);
        memcpy(&extra[to], &extra[off], len * sizeof(CovisExtra));
        pool.touch(to * 2, len * 2);
    }
    dead += have;
    seg_cap[p] = (uint32_t)need;
    set_ptab(p, 0, (int32_t)to);
    return (int)(to + len);
}

/* segments back to back in point-slot order, each with its capacity; both arrays go up whole afterwards */
void CovisStore::compact() {
    if (dead * 2 <= used) return;
    std::vector<int32_t> w(cap * 2, 0);
    std::vector<CovisExtra> ex(cap);
    size_t to = 0;
    for (size_t p = 0; p < mp_id.size(); p++) {
        if (!seg_cap[p]) continue;
        const size_t off = (uint32_t)ptab.w[p * 4], len = (size_t)ptab.w[p * 4 + 1];
        if (len) {
            memcpy(&w[to * 2], &pool.w[off * 2], len * 8);
            memcpy(&ex[to], &extra[off], len * sizeof(CovisExtra));
        }
        ptab.w[p * 4] = (int32_t)to;
        to += seg_cap[p];
    }
    pool.w.swap(w);
    extra.swap(ex);
    used = to;
    dead = 0;
    pool.all = ptab.all = true;
    n_compact++;
}

static int32_t covis_level(const CovisExtra& e) { /* localmapping.cpp:1024-1036 */
    if (e.lvlL < 0) return e.lvlR;
    if (e.lvlR < 0) return e.lvlL;
    return std::min(e.lvlL, e.lvlR);
}

int CovisStore::add_observation(int64_t mp, int64_t kf, int32_t idx, int is_right, int level, int stereo) {
    auto pi = mp_slot.find(mp);
    auto ki = kf_slot.find(kf);
    if (pi == mp_slot.end() || ki == kf_slot.end()) return fail("covis add_observation: unknown MapPoint or keyframe");
    if (idx < 0 || level < 0 || level > 63) return fail("covis add_observation: idx >= 0 and level in [0, 63]");
    const int32_t p = pi->second, k = ki->second;
    size_t off = (uint32_t)ptab.w[(size_t)p * 4], len = (size_t)ptab.w[(size_t)p * 4 + 1];
    size_t r = 0;
    while (r < len && pool.w[(off + r) * 2] != k) r++;
    size_t at = off + r;
    if (r == len) { /* mappoint.cpp:145-147 */
        at = (size_t)reserve_record(p);
        pool.w[at * 2] = k;
        extra[at] = CovisExtra{-1, -1, -1, -1, 0, 0};
        kf_refs[k]++;
        n_records++;
        set_ptab(p, 1, (int32_t)len + 1);
    }
    CovisExtra& e = extra[at];
    if (is_right) { /* :149-154 */
        e.idxR = idx;
        e.lvlR = (int8_t)level;
    } else {
        e.idxL = idx;
        e.lvlL = (int8_t)level;
        e.stereo = stereo ? 1 : 0;
    }
    pool.w[at * 2 + 1] = covis_level(e);
    pool.touch(at * 2, 2);
    set_ptab(p, 2, ptab.w[(size_t)p * 4 + 2] + (stereo ? 2 : 1)); /* :158-161 */
    compact();
    return VSLAM_OK;
}

int CovisStore::erase_observation(int64_t mp, int64_t kf, int* became_bad) {
    if (became_bad) *became_bad = 0;
    auto pi = mp_slot.find(mp);
    auto ki = kf_slot.find(kf);
    if (pi == mp_slot.end() || ki == kf_slot.end()) return fail("covis erase_observation: unknown MapPoint or keyframe");
    const int32_t p = pi->second, k = ki->second;
    const size_t off = (uint32_t)ptab.w[(size_t)p * 4], len = (size_t)ptab.w[(size_t)p * 4 + 1];
    size_t r = 0;
    while (r < len && pool.w[(off + r) * 2] != k) r++;
    if (r == len) return VSLAM_OK; /* mappoint.cpp:169 */
    const CovisExtra e = extra[off + r];
    int32_t nobs = ptab.w[(size_t)p * 4 + 2];
    if (e.idxL != -1) nobs -= e.stereo ? 2 : 1; /* :174-179 */
    if (e.idxR != -1) nobs--;                   /* :180-182 */
    if (r + 1 < len) {
        pool.w[(off + r) * 2] = pool.w[(off + len - 1) * 2];
        pool.w[(off + r) * 2 + 1] = pool.w[(off + len - 1) * 2 + 1];
        extra[off + r] = extra[off + len - 1];
        pool.touch((off + r) * 2, 2);
    }
    kf_refs[k]--;
    n_records--;
    set_ptab(p, 1, (int32_t)len - 1);
    set_ptab(p, 2, nobs);
    if (nobs <= 2) { /* :190-196, :211-220 */
        drop_records(p);
        drop_segment(p);
        set_ptab(p, 3, ptab.w[(size_t)p * 4 + 3] | COVIS_BAD);
        if (became_bad) *became_bad = 1;
        compact();
    }
    return VSLAM_OK;
}

int CovisStore::clear_point(int64_t mp) {
    auto pi = mp_slot.find(mp);
    if (pi == mp_slot.end()) return fail("covis clear_point: unknown MapPoint");
    const int32_t p = pi->second;
    drop_records(p);
    drop_segment(p);
    set_ptab(p, 3, ptab.w[(size_t)p * 4 + 3] | COVIS_BAD);
    compact();
    return VSLAM_OK;
}

int CovisStore::erase_point(int64_t mp) {
    auto pi = mp_slot.find(mp);
    if (pi == mp_slot.end()) return fail("covis erase_point: unknown MapPoint");
    const int32_t p = pi->second;
    drop_records(p);
    drop_segment(p);
    set_ptab(p, 2, 0);
    set_ptab(p, 3, 0);
    mp_slot.erase(pi);
    mp_free.push_back(p);
    compact();
    return VSLAM_OK;
}

int CovisStore::clear_map(int32_t map) {
    std::vector<int64_t> kfs, mps;
    for (size_t s = 0; s < kf_id.size(); s++)
        if ((ktab[s * 4 + 2] & COVIS_ALIVE) && ktab[s * 4 + 1] == map) kfs.push_back(kf_id[s]);
    for (size_t p = 0; p < mp_id.size(); p++) {
        if (!(ptab.w[p * 4 + 3] & COVIS_ALIVE)) continue;
        const size_t off = (uint32_t)ptab.w[p * 4], len = (size_t)ptab.w[p * 4 + 1];
        for (size_t i = 0; i < len; i++) {
            const int32_t k = pool.w[(off + i) * 2];
            if (ktab[(size_t)k * 4 + 1] == map) {
                mps.push_back(mp_id[p]);
                break;
            }
        }
    }
    for (int64_t m : mps) erase_point(m);
    for (int64_t k : kfs) erase_keyframe(k);
    return VSLAM_OK;
}

int CovisStore::clear() {
    const size_t keep = cap;
    const unsigned long long g = n_grow, c = n_compact;
    *this = CovisStore(keep);
    n_grow = g;
    n_compact = c;
    return VSLAM_OK;
}

int CovisStore::get_point(int64_t mp, int cap_obs, int* n_obs, int* bad, vslam_covis_obs* obs, int* n_rec) const {
    auto pi = mp_slot.find(mp);
    if (pi == mp_slot.end() || cap_obs < 0) {
        err = "covis get_point: unknown MapPoint";
        return VSLAM_ERR_INVALID;
    }
    const size_t p = (size_t)pi->second;
    const size_t off = (uint32_t)ptab.w[p * 4], len = (size_t)ptab.w[p * 4 + 1];
    if (n_obs) *n_obs = ptab.w[p * 4 + 2];
    if (bad) *bad = (ptab.w[p * 4 + 3] & COVIS_BAD) ? 1 : 0;
    if (n_rec) *n_rec = (int)len;
    if (!obs || !len) return VSLAM_OK;
    if ((size_t)cap_obs < len) {
        err = "covis get_point: more observations than the caller's array holds";
        return VSLAM_ERR_CAPACITY;
    }
    std::vector<size_t> at(len);
    for (size_t i = 0; i < len; i++) at[i] = off + i;
    std::sort(at.begin(), at.end(), [&](size_t a, size_t b) { return kf_key[pool.w[a * 2]] < kf_key[pool.w[b * 2]]; });
    for (size_t i = 0; i < len; i++) {
        const CovisExtra& e = extra[at[i]];
        obs[i] = vslam_covis_obs{kf_id[pool.w[at[i] * 2]], e.idxL, e.idxR, e.lvlL, e.lvlR, e.stereo, 0};
    }
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ the queries from the shadow */
int covis_jobs_ok(int n_jobs, const vslam_covis_job* jobs, std::string& err) {
    if (n_jobs < 1 || n_jobs > VSLAM_COVIS_MAX_JOBS || !jobs) {
        err = "covis connections: 1..VSLAM_COVIS_MAX_JOBS jobs";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < n_jobs; j++) {
        const vslam_covis_job& J = jobs[j];
        if (J.n < 0 || J.n > VSLAM_COVIS_MAX_LIST || (J.n && !J.mp_ids) ||
            (J.mode != VSLAM_COVIS_CONNECTIONS && J.mode != VSLAM_COVIS_VOTE)) {
            err = "covis connections: a job's mode is CONNECTIONS or VOTE and its list holds 0..VSLAM_COVIS_MAX_LIST ids";
            return VSLAM_ERR_INVALID;
        }
    }
    return VSLAM_OK;
}

int covis_cull_jobs_ok(int n_jobs, const vslam_covis_cull_job* jobs, int th_obs, std::string& err) {
    if (n_jobs < 1 || n_jobs > VSLAM_COVIS_MAX_JOBS || !jobs || th_obs < 0) {
        err = "covis culling: 1..VSLAM_COVIS_MAX_JOBS jobs, th_obs >= 0";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < n_jobs; j++) {
        const vslam_covis_cull_job& J = jobs[j];
        if (J.n < 0 || J.n > VSLAM_COVIS_MAX_LIST || (J.n && (!J.mp_ids || !J.levels))) {
            err = "covis culling: a job's list holds 0..VSLAM_COVIS_MAX_LIST ids and levels";
            return VSLAM_ERR_INVALID;
        }
    }
    return VSLAM_OK;
}

int CovisStore::connections(int n_jobs, const vslam_covis_job* jobs, vslam_covis_result* res,
                            std::vector<int64_t>& counter_kf, std::vector<int32_t>& counter_n,
                            std::vector<int64_t>& ordered_kf, std::vector<int32_t>& ordered_w) {
    if (int rc = covis_jobs_ok(n_jobs, jobs, err)) return rc;
    if (!res) return fail("covis connections: invalid arguments");
    refresh_ranks();
    counter_kf.clear();
    counter_n.clear();
    ordered_kf.clear();
    ordered_w.clear();
    std::vector<int32_t> hist(korder.size());
    for (int j = 0; j < n_jobs; j++) {
        const vslam_covis_job& J = jobs[j];
        vslam_covis_result R{0, 0, 0, 0, -1, 0, 0};
        int32_t self = -1;
        if (J.mode == VSLAM_COVIS_CONNECTIONS) {
            auto ki = kf_slot.find(J.self_kf);
            if (ki == kf_slot.end()) R.error |= 2;
            else self = ki->second;
        }
        for (int i = 0; i < J.n; i++)
            if (J.mp_ids[i] != -1 && !mp_slot.count(J.mp_ids[i])) R.error |= 1;
        if (R.error) {
            res[j] = R;
            continue;
        }
        std::fill(hist.begin(), hist.end(), 0);
        for (int i = 0; i < J.n; i++) {
            if (J.mp_ids[i] == -1) continue;                   /* keyframe.cpp:367 */
            const size_t p = (size_t)mp_slot.find(J.mp_ids[i])->second;
            if (ptab.w[p * 4 + 3] & COVIS_BAD) continue;       /* :370 */
            if (J.min_obs > 0 ? ptab.w[p * 4 + 2] >= J.min_obs : true) R.n_tracked++; /* :329-333 */
            const size_t off = (uint32_t)ptab.w[p * 4], len = (size_t)ptab.w[p * 4 + 1];
            for (size_t r = 0; r < len; r++) {
                const int32_t k = pool.w[(off + r) * 2];
                const int32_t* K = &ktab[(size_t)k * 4];
                if (J.mode == VSLAM_COVIS_CONNECTIONS && (k == self || (K[2] & COVIS_BAD) || K[1] != J.map_id)) continue; /* :377 */
                hist[K[0]]++;
            }
        }
        const size_t c0 = counter_kf.size();
        for (size_t r = 0; r < korder.size(); r++) { /* ascending order_key */
            const int32_t k = korder[r], n = hist[r];
            if (!n) continue;
            if (J.mode == VSLAM_COVIS_VOTE && (ktab[(size_t)k * 4 + 2] & COVIS_BAD)) continue; /* tracking.cpp:3365 */
            if (n > R.n_max) {                                                                /* :402, :3368 */
                R.n_max = n;
                R.kf_max = kf_id[k];
            }
            counter_kf.push_back(kf_id[k]);
            counter_n.push_back(n);
        }
        R.n_counter = (int32_t)(counter_kf.size() - c0);
        if (J.mode == VSLAM_COVIS_CONNECTIONS && R.n_counter) {
            const size_t o0 = ordered_kf.size();
            for (size_t i = counter_kf.size(); i-- > c0;) /* the counter read backwards: descending order_key */
                if (counter_n[i] >= COVIS_TH_WEIGHT) {
                    ordered_kf.push_back(counter_kf[i]);
                    ordered_w.push_back(counter_n[i]);
                }
            if (ordered_kf.size() == o0) { /* :414-418 */
                ordered_kf.push_back(R.kf_max);
                ordered_w.push_back(R.n_max);
            } else {
                /* descending (count, order_key): the entries stand in descending key, a stable sort by count keeps that */
                std::vector<size_t> ix(ordered_kf.size() - o0);
                for (size_t i = 0; i < ix.size(); i++) ix[i] = o0 + i;
                std::stable_sort(ix.begin(), ix.end(), [&](size_t a, size_t b) { return ordered_w[a] > ordered_w[b]; });
                std::vector<int64_t> k2(ix.size());
                std::vector<int32_t> w2(ix.size());
                for (size_t i = 0; i < ix.size(); i++) {
                    k2[i] = ordered_kf[ix[i]];
                    w2[i] = ordered_w[ix[i]];
                }
                std::copy(k2.begin(), k2.end(), ordered_kf.begin() + (long)o0);
                std::copy(w2.begin(), w2.end(), ordered_w.begin() + (long)o0);
            }
            R.n_ordered = (int32_t)(ordered_kf.size() - o0);
        }
        res[j] = R;
    }
    return VSLAM_OK;
}

int CovisStore::culling(int n_jobs, const vslam_covis_cull_job* jobs, int th_obs, vslam_covis_cull_result* res) {
    if (int rc = covis_cull_jobs_ok(n_jobs, jobs, th_obs, err)) return rc;
    if (!res) return fail("covis culling: invalid arguments");
    for (int j = 0; j < n_jobs; j++) {
        const vslam_covis_cull_job& J = jobs[j];
        vslam_covis_cull_result R{0, 0, 0, 0};
        auto ki = kf_slot.find(J.kf_id);
        if (ki == kf_slot.end()) R.error |= 2;
        for (int i = 0; i < J.n; i++)
            if (J.mp_ids[i] != -1 && !mp_slot.count(J.mp_ids[i])) R.error |= 1;
        if (R.error) {
            res[j] = R;
            continue;
        }
        const int32_t self = ki->second;
        for (int i = 0; i < J.n; i++) {
            if (J.mp_ids[i] == -1) continue; /* localmapping.cpp:999, :1003-1007 */
            const size_t p = (size_t)mp_slot.find(J.mp_ids[i])->second;
            if (ptab.w[p * 4 + 3] & COVIS_BAD) continue; /* :1001 */
            R.n_mps++;
            if (ptab.w[p * 4 + 2] <= th_obs) continue; /* :1010 */
            const size_t off = (uint32_t)ptab.w[p * 4], len = (size_t)ptab.w[p * 4 + 1];
            int n = 0;
            for (size_t r = 0; r < len; r++)
                if (pool.w[(off + r) * 2] != self && pool.w[(off + r) * 2 + 1] <= J.levels[i] + 1) n++; /* :1020, :1038 */
            if (n > th_obs) R.n_redundant++; /* :1045 */
        }
        res[j] = R;
    }
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ the GPU-free handle (libvslam_host.so; the product
 * library exports it too).  vslamh_covis_last_error: the text of the handle's last failure. */
struct vslamh_covis {
    CovisStore s;
    std::vector<int64_t> counter_kf, ordered_kf;
    std::vector<int32_t> counter_n, ordered_w;
    std::vector<vslam_covis_result> res;
    explicit vslamh_covis(size_t n) : s(n) {}
};

extern "C" {
vslamh_covis* vslamh_covis_create(int initial_entries) { return initial_entries < 0 ? nullptr : new vslamh_covis((size_t)initial_entries); }
void vslamh_covis_destroy(vslamh_covis* c) { delete c; }
const char* vslamh_covis_last_error(vslamh_covis* c) { return c ? c->s.err.c_str() : "null handle"; }
int vslamh_covis_add_keyframe(vslamh_covis* c, int64_t kf, int32_t map, uint64_t key) { return c ? c->s.add_keyframe(kf, map, key) : VSLAM_ERR_INVALID; }
int vslamh_covis_add_keyframes(vslamh_covis* c, int n, const int64_t* kf, const int32_t* map, const uint64_t* key) {
    return c ? c->s.add_keyframes(n, kf, map, key) : VSLAM_ERR_INVALID;
}
int vslamh_covis_set_keyframe_bad(vslamh_covis* c, int64_t kf) { return c ? c->s.set_keyframe_bad(kf) : VSLAM_ERR_INVALID; }
int vslamh_covis_set_keyframe_map(vslamh_covis* c, int64_t kf, int32_t map) { return c ? c->s.set_keyframe_map(kf, map) : VSLAM_ERR_INVALID; }
int vslamh_covis_erase_keyframe(vslamh_covis* c, int64_t kf) { return c ? c->s.erase_keyframe(kf) : VSLAM_ERR_INVALID; }
int vslamh_covis_add_point(vslamh_covis* c, int64_t mp) { return c ? c->s.add_point(mp) : VSLAM_ERR_INVALID; }
int vslamh_covis_add_observation(vslamh_covis* c, int64_t mp, int64_t kf, int32_t idx, int is_right, int level, int stereo) {
    return c ? c->s.add_observation(mp, kf, idx, is_right, level, stereo) : VSLAM_ERR_INVALID;
}
int vslamh_covis_erase_observation(vslamh_covis* c, int64_t mp, int64_t kf, int* became_bad) {
    return c ? c->s.erase_observation(mp, kf, became_bad) : VSLAM_ERR_INVALID;
}
int vslamh_covis_clear_point(vslamh_covis* c, int64_t mp) { return c ? c->s.clear_point(mp) : VSLAM_ERR_INVALID; }
int vslamh_covis_erase_point(vslamh_covis* c, int64_t mp) { return c ? c->s.erase_point(mp) : VSLAM_ERR_INVALID; }
int vslamh_covis_clear_map(vslamh_covis* c, int32_t map) { return c ? c->s.clear_map(map) : VSLAM_ERR_INVALID; }
int vslamh_covis_clear(vslamh_covis* c) { return c ? c->s.clear() : VSLAM_ERR_INVALID; }
int vslamh_covis_size(vslamh_covis* c, int* n_kf, int* n_mp, long long* n_obs) {
    if (!c) return VSLAM_ERR_INVALID;
    if (n_kf) *n_kf = (int)c->s.kf_slot.size();
    if (n_mp) *n_mp = (int)c->s.mp_slot.size();
    if (n_obs) *n_obs = (long long)c->s.n_records;
    return VSLAM_OK;
}
int vslamh_covis_stats(vslamh_covis* c, long long* capacity, long long* used, int* n_growths, int* n_compactions) {
    if (!c) return VSLAM_ERR_INVALID;
    if (capacity) *capacity = (long long)c->s.cap;
    if (used) *used = (long long)c->s.used;
    if (n_growths) *n_growths = (int)c->s.n_grow;
    if (n_compactions) *n_compactions = (int)c->s.n_compact;
    return VSLAM_OK;
}
int vslamh_covis_get_point(vslamh_covis* c, int64_t mp, int cap, int* n_obs, int* bad, vslam_covis_obs* obs, int* n_records) {
    return c ? c->s.get_point(mp, cap, n_obs, bad, obs, n_records) : VSLAM_ERR_INVALID;
}
int vslamh_covis_connections(vslamh_covis* c, int n_jobs, const vslam_covis_job* jobs, vslam_covis_result* results) {
    if (!c) return VSLAM_ERR_INVALID;
    c->res.clear();
    const int rc = c->s.connections(n_jobs, jobs, results, c->counter_kf, c->counter_n, c->ordered_kf, c->ordered_w);
    if (!rc) c->res.assign(results, results + n_jobs);
    return rc;
}
int vslamh_covis_connections_lists(vslamh_covis* c, int job, int64_t* counter_kf, int32_t* counter_n, int64_t* ordered_kf,
                                   int32_t* ordered_w) {
    if (!c || job < 0 || job >= (int)c->res.size()) return VSLAM_ERR_INVALID;
    size_t c0 = 0, o0 = 0;
    for (int j = 0; j < job; j++) {
        c0 += (size_t)c->res[j].n_counter;
        o0 += (size_t)c->res[j].n_ordered;
    }
    const size_t nc = (size_t)c->res[job].n_counter, no = (size_t)c->res[job].n_ordered;
    if (counter_kf && nc) memcpy(counter_kf, &c->counter_kf[c0], nc * 8);
    if (counter_n && nc) memcpy(counter_n, &c->counter_n[c0], nc * 4);
    if (ordered_kf && no) memcpy(ordered_kf, &c->ordered_kf[o0], no * 8);
    if (ordered_w && no) memcpy(ordered_w, &c->ordered_w[o0], no * 4);
    return VSLAM_OK;
}
int vslamh_covis_culling(vslamh_covis* c, int n_jobs, const vslam_covis_cull_job* jobs, int th_obs, vslam_covis_cull_result* results) {
    return c ? c->s.culling(n_jobs, jobs, th_obs, results) : VSLAM_ERR_INVALID;
}
}
