// mem_owner.cpp -- the owning buffer of vi_slam_amd/csrc/vslam_mem.h over a counting space: every live block is
// recorded, an allocation fails on demand, and a free of a pointer that is not live aborts.  The checks are the
// program's own bookkeeping; built with plain g++ and run by tests/test_host_logic.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../vi_slam_amd/csrc/vslam_mem.h"

struct CountingSpace {
    static std::map<void*, size_t> live;
    static long allocs, frees, uploads;
    static bool fail_next;
    static int alloc(void** p, size_t bytes) {
        if (fail_next) {
            fail_next = false;
            return VSLAM_ERR_HIP;
        }
        *p = malloc(bytes ? bytes : 1);
        live[*p] = bytes;
        allocs++;
        return VSLAM_OK;
    }
    static void free(void* p, size_t bytes) {
        auto it = live.find(p);
        if (it == live.end() || it->second != bytes) {
            fprintf(stderr, "FATAL: free of %p (%zu bytes), which is not a live block of that size\n", p, bytes);
            abort();
        }
        live.erase(it);
        frees++;
        ::free(p);
    }
    static int upload(void* dst, const void* src, size_t bytes) {
        memcpy(dst, src, bytes);
        uploads++;
        return VSLAM_OK;
    }
};
std::map<void*, size_t> CountingSpace::live;
long CountingSpace::allocs = 0, CountingSpace::frees = 0, CountingSpace::uploads = 0;
bool CountingSpace::fail_next = false;

using S = CountingSpace;
template <class T>
using buf = vslam_buf<T, CountingSpace>;

static int g_bad = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_bad++;                                             \
        }                                                        \
    } while (0)

struct Group { /* the shape of vslam_fe::PyrGroupCtx: plain fields and a buffer, move-only */
    int l0 = 0;
    buf<uint32_t> tiles;
};

int main() {
    { /* ensure: grow-only, contents not kept */
        buf<uint32_t> b;
        CHECK(!b.get() && b.bytes() == 0 && b.count() == 0 && !b);
        CHECK(b.ensure(100) == VSLAM_OK && b.count() == 100 && b.bytes() == 400 && S::live.size() == 1);
        uint32_t* const first = b;
        const long a0 = S::allocs, f0 = S::frees;
        CHECK(b.ensure(40) == VSLAM_OK && b.get() == first && b.count() == 100); /* smaller: no allocation, same address */
        CHECK(b.ensure(100) == VSLAM_OK && b.get() == first);
        CHECK(S::allocs == a0 && S::frees == f0);
        CHECK(b.ensure(101) == VSLAM_OK && b.count() == 101); /* larger: the old block is freed exactly once */
        CHECK(S::allocs == a0 + 1 && S::frees == f0 + 1 && S::live.size() == 1 && S::live.count(b.get()) == 1);
        /* a failed allocation: empty, size 0, the error returned; the old block is gone, once */
        S::fail_next = true;
        CHECK(b.ensure(500) == VSLAM_ERR_HIP && !b.get() && b.bytes() == 0 && S::live.empty() && S::frees == f0 + 2);
        CHECK(b.ensure(8) == VSLAM_OK && b.count() == 8 && S::live.size() == 1); /* a later ensure succeeds */
        /* alloc: always a fresh block */
        const long a1 = S::allocs, f1 = S::frees;
        CHECK(b.alloc(4) == VSLAM_OK && b.count() == 4 && S::allocs == a1 + 1 && S::frees == f1 + 1);
        b[3] = 7u; /* the conversion: indexing and arithmetic as with a raw pointer */
        CHECK(*(b + 3) == 7u && ((const uint8_t*)b)[12] == 7u);
        b.release();
        b.release(); /* twice is harmless */
        CHECK(!b.get() && b.bytes() == 0 && S::live.empty() && S::frees == f1 + 2);
    }
    { /* move and swap */
        buf<uint8_t> a, b;
        CHECK(a.alloc(16) == VSLAM_OK && b.alloc(32) == VSLAM_OK);
        uint8_t *pa = a, *pb = b;
        buf<uint8_t> c(std::move(a)); /* move-construct: the source is empty */
        CHECK(!a.get() && a.bytes() == 0 && c.get() == pa && c.bytes() == 16 && S::live.size() == 2);
        const long f0 = S::frees;
        b = std::move(c); /* move-assign: the target's former block is freed once, the source is empty */
        CHECK(S::frees == f0 + 1 && !c.get() && c.bytes() == 0 && b.get() == pa && b.bytes() == 16);
        CHECK(S::live.size() == 1 && S::live.count(pb) == 0);
        CHECK(c.alloc(5) == VSLAM_OK);
        uint8_t* pc = c;
        b.swap(c);
        CHECK(b.get() == pc && b.bytes() == 5 && c.get() == pa && c.bytes() == 16 && S::frees == f0 + 1);
        b = std::move(b); /* self-assignment keeps the block */
        CHECK(b.get() == pc && S::live.size() == 2);
    }
    CHECK(S::live.empty());
    { /* upload: a table into an allocation of its own; an empty table has an address too */
        buf<uint16_t> t;
        const uint16_t src[3] = {1, 2, 3};
        CHECK(vslam_upload(t, src, sizeof(src)) == VSLAM_OK && t.bytes() == 6 && t[2] == 3 && S::uploads == 1);
        buf<double> z;
        CHECK(vslam_upload(z, nullptr, 0) == VSLAM_OK && z.get() && z.bytes() >= 4 && S::uploads == 1);
        S::fail_next = true;
        CHECK(vslam_upload(t, src, sizeof(src)) == VSLAM_ERR_HIP && !t.get() && S::uploads == 1);
    }
    CHECK(S::live.empty());
    { /* a vector of structs that hold a buffer grows past its capacity and is cleared (a failed pyramid plan) */
        std::vector<Group> groups;
        std::vector<uint32_t*> addr;
        for (int i = 0; i < 37; i++) {
            Group g;
            g.l0 = i;
            CHECK(g.tiles.alloc(3 + i) == VSLAM_OK);
            g.tiles[0] = (uint32_t)i;
            addr.push_back(g.tiles);
            groups.push_back(std::move(g));
        }
        CHECK(S::live.size() == 37 && S::frees + 37 == S::allocs);
        for (int i = 0; i < 37; i++) CHECK(groups[i].l0 == i && groups[i].tiles.get() == addr[i] && groups[i].tiles[0] == (uint32_t)i);
        groups.clear();
        CHECK(S::live.empty());
    }
    CHECK(S::live.empty() && S::allocs == S::frees);
    if (g_bad) return 1;
    printf("mem_owner ok: %ld allocations, %ld frees, 0 live\n", S::allocs, S::frees);
    return 0;
}
