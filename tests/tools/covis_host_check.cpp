/* covis_host_check.cpp -- stand-alone replay of the covisibility bookkeeping and host twins (vslam_covis_host.cpp), meant to be
 * built with -fsanitize=address,undefined: the pool's growth, compaction and erase paths are where a memory error would
 * live.  Reads the text files of tests/tools/dump_covis_cases.py and compares every answer with the dumped one.
 *   g++ -std=c++17 -fsanitize=address,undefined -I include tests/tools/covis_host_check.cpp vi_slam_amd/csrc/vslam_covis_host.cpp */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../vi_slam_amd/csrc/vslam_covis.h"

static int fails = 0;
#define EXPECT(cond, what)                                                         \
    do {                                                                           \
        if (!(cond)) {                                                             \
            if (fails++ < 20) fprintf(stderr, "%s:%d: %s\n", file, line_no, what); \
        }                                                                          \
    } while (0)

static std::vector<long long> rest(std::istringstream& in, size_t n) {
    std::vector<long long> v(n);
    for (size_t i = 0; i < n; i++) in >> v[i];
    return v;
}

static int run_file(const char* file) {
    std::ifstream f(file);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", file);
        return 1;
    }
    CovisStore* s = nullptr;
    std::string line;
    int line_no = 0;
    long n_ops = 0, n_checks = 0;
    while (std::getline(f, line)) {
        line_no++;
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "create") {
            long long n;
            in >> n;
            delete s;
            s = new CovisStore((size_t)n);
        } else if (what == "op") {
            std::string name;
            int want;
            in >> name >> want;
            std::vector<long long> a;
            for (long long v; in >> v;) a.push_back(v);
            a.resize(8, 0);
            int rc = 12345, bad = 0;
            if (name == "add_keyframe") rc = s->add_keyframe(a[0], (int32_t)a[1], (uint64_t)a[2]);
            else if (name == "set_keyframe_bad") rc = s->set_keyframe_bad(a[0]);
            else if (name == "set_keyframe_map") rc = s->set_keyframe_map(a[0], (int32_t)a[1]);
            else if (name == "erase_keyframe") rc = s->erase_keyframe(a[0]);
            else if (name == "add_point") rc = s->add_point(a[0]);
            else if (name == "add_observation") rc = s->add_observation(a[0], a[1], (int32_t)a[2], (int)a[3], (int)a[4], (int)a[5]);
            else if (name == "erase_observation") rc = s->erase_observation(a[0], a[1], &bad);
            else if (name == "clear_point") rc = s->clear_point(a[0]);
            else if (name == "erase_point") rc = s->erase_point(a[0]);
            else if (name == "clear_map") rc = s->clear_map((int32_t)a[0]);
            else if (name == "clear") rc = s->clear();
            EXPECT(rc == want, "a mutator's return code");
            n_ops++;
        } else if (what == "point") {
            long long mp, nobs, bad, n;
            in >> mp >> nobs >> bad >> n;
            const std::vector<long long> w = rest(in, (size_t)n * 6);
            std::vector<vslam_covis_obs> obs((size_t)n + 1);
            int g_nobs = -1, g_bad = -1, g_n = -1;
            const int rc = s->get_point(mp, (int)n, &g_nobs, &g_bad, obs.data(), &g_n);
            EXPECT(rc == 0 && g_nobs == nobs && g_bad == bad && g_n == n, "get_point: nObs, bad flag or count");
            for (long long i = 0; i < n && g_n == n; i++) {
                const vslam_covis_obs& o = obs[(size_t)i];
                const long long* e = &w[(size_t)i * 6];
                EXPECT(o.kf_id == e[0] && o.left_idx == e[1] && o.right_idx == e[2] && o.left_level == e[3] &&
                           o.right_level == e[4] && o.stereo == e[5], "get_point: an observation");
            }
            n_checks++;
        } else if (what == "size") {
            long long k, m, o;
            in >> k >> m >> o;
            EXPECT((long long)s->kf_slot.size() == k && (long long)s->mp_slot.size() == m && (long long)s->n_records == o, "size");
        } else if (what == "stats") {
            long long g, c;
            in >> g >> c;
            EXPECT((long long)s->n_grow >= g && (long long)s->n_compact >= c && s->used <= s->cap, "growths / compactions");
            printf("%s: capacity %zu used %zu growths %llu compactions %llu\n", file, s->cap, s->used, s->n_grow, s->n_compact);
        } else if (what == "conn") {
            vslam_covis_job J{};
            long long self;
            in >> J.mode >> self >> J.map_id >> J.min_obs >> J.n;
            J.self_kf = self;
            std::vector<long long> idv = rest(in, (size_t)J.n);
            std::vector<int64_t> ids(idv.begin(), idv.end());
            J.mp_ids = ids.data();
            std::string bar;
            long long err, kf_max, n_max, n_tracked, nc, no;
            in >> bar >> err >> kf_max >> n_max >> n_tracked >> nc;
            const std::vector<long long> ck = rest(in, (size_t)nc), cn = rest(in, (size_t)nc);
            in >> no;
            const std::vector<long long> ok = rest(in, (size_t)no), ow = rest(in, (size_t)no);
            vslam_covis_result R{};
            std::vector<int64_t> gk, gok;
            std::vector<int32_t> gn, gow;
            const int rc = s->connections(1, &J, &R, gk, gn, gok, gow);
            EXPECT(rc == 0 && R.error == err && R.kf_max == kf_max && R.n_max == n_max && R.n_tracked == n_tracked &&
                       R.n_counter == nc && R.n_ordered == no && (long long)gk.size() == nc && (long long)gok.size() == no,
                   "connections: the job's result");
            for (size_t i = 0; i < gk.size() && (long long)gk.size() == nc; i++) EXPECT(gk[i] == ck[i] && gn[i] == cn[i], "connections: counter");
            for (size_t i = 0; i < gok.size() && (long long)gok.size() == no; i++) EXPECT(gok[i] == ok[i] && gow[i] == ow[i], "connections: ordered list");
            n_checks++;
        } else if (what == "cull") {
            vslam_covis_cull_job J{};
            long long kf, th;
            in >> kf >> th >> J.n;
            J.kf_id = kf;
            std::vector<long long> idv = rest(in, (size_t)J.n), lvv = rest(in, (size_t)J.n);
            std::vector<int64_t> ids(idv.begin(), idv.end());
            std::vector<int32_t> lv(lvv.begin(), lvv.end());
            J.mp_ids = ids.data();
            J.levels = lv.data();
            std::string bar;
            long long err, n_mps, n_red;
            in >> bar >> err >> n_mps >> n_red;
            vslam_covis_cull_result R{};
            const int rc = s->culling(1, &J, (int)th, &R);
            EXPECT(rc == 0 && R.error == err && R.n_mps == n_mps && R.n_redundant == n_red, "culling: the job's result");
            n_checks++;
        } else if (!what.empty()) {
            EXPECT(false, "unknown line");
        }
    }
    delete s;
    printf("%s: %ld calls, %ld comparisons\n", file, n_ops, n_checks);
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++)
        if (run_file(argv[i])) return 2;
    if (fails) fprintf(stderr, "%d mismatches\n", fails);
    return fails ? 1 : 0;
}
