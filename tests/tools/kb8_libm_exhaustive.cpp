/* kb8_libm_exhaustive.cpp -- compares the libm restatements of vi_slam_amd/csrc/vslam_kb8.h and vslam_trig.h with the
 * platform libm, bit for bit, on the CPU:
 *   atanf        all 2^32 inputs
 *   tanf         all |x| < 3*pi/4
 *   sinf, cosf   all |x| <= pi
 *   atan2f       at least 200 M pairs: half raw bit patterns, half uniform in [-10, 10]^2 (fixed seed)
 * NaN results count as equal when both are NaN.  Prints one line per function and the glibc version; exit status 1 when
 * anything differs.
 *
 *   g++ -O2 -std=c++17 -ffp-contract=off -pthread tests/tools/kb8_libm_exhaustive.cpp -o kb8_libm_exhaustive
 *   ./kb8_libm_exhaustive [stride [threads [report.txt]]]      stride 1 = everything; 1024 for a sanitizer build
 */
#include <gnu/libc-version.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../vi_slam_amd/csrc/vslam_kb8.h"

using vslam_kb8::as_f32;
using vslam_trig::as_u32;

static int g_failed = 0;
static bool same(float a, float b) { return as_u32(a) == as_u32(b) || (a != a && b != b); }

template <typename Fn>
static void run(const char* name, uint64_t total, int nthreads, FILE* out, Fn body) {
    std::atomic<uint64_t> bad{0}, done{0};
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++)
        th.emplace_back([&, t] {
            uint64_t b = 0, d = 0;
            const uint64_t lo = total * t / nthreads, hi = total * (t + 1) / nthreads;
            for (uint64_t i = lo; i < hi; i++) body(i, &b, &d);
            bad += b;
            done += d;
        });
    for (auto& x : th) x.join();
    fprintf(out, "%-8s %12llu inputs  %llu mismatches\n", name, (unsigned long long)done.load(), (unsigned long long)bad.load());
    fflush(out);
    if (bad.load()) g_failed = 1;
}

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    const uint64_t stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int nthreads = argc > 2 ? atoi(argv[2]) : 8;
    FILE* out = argc > 3 ? fopen(argv[3], "a") : stdout;
    if (!out || stride < 1 || nthreads < 1) return 2;
    fprintf(out, "glibc %s, stride %llu\n", gnu_get_libc_version(), (unsigned long long)stride);
    const uint32_t lim_tan = 0x4016cbe4u, lim_pi = 0x40490fdbu; /* first |x| outside: 3*pi/4; (float)pi itself is inside */
    run("atanf", (1ull << 32) / stride, nthreads, out, [&](uint64_t i, uint64_t* b, uint64_t* d) {
        const float x = as_f32((uint32_t)(i * stride));
        *b += !same(vslam_kb8::glibc_atanf(x), atanf(x));
        ++*d;
    });
    run("tanf", (1ull << 32) / stride, nthreads, out, [&](uint64_t i, uint64_t* b, uint64_t* d) {
        const uint32_t u = (uint32_t)(i * stride);
        if ((u & 0x7fffffffu) >= lim_tan) return;
        const float x = as_f32(u);
        *b += !same(vslam_kb8::glibc_tanf(x), tanf(x));
        ++*d;
    });
    run("sinf", (1ull << 32) / stride, nthreads, out, [&](uint64_t i, uint64_t* b, uint64_t* d) {
        const uint32_t u = (uint32_t)(i * stride);
        if ((u & 0x7fffffffu) > lim_pi) return;
        const float x = as_f32(u);
        *b += !same(vslam_trig::glibc_sinf(x), sinf(x));
        ++*d;
    });
    run("cosf", (1ull << 32) / stride, nthreads, out, [&](uint64_t i, uint64_t* b, uint64_t* d) {
        const uint32_t u = (uint32_t)(i * stride);
        if ((u & 0x7fffffffu) > lim_pi) return;
        const float x = as_f32(u);
        *b += !same(vslam_trig::glibc_cosf(x), cosf(x));
        ++*d;
    });
    const uint64_t npairs = (208ull << 20) / stride;
    run("atan2f", npairs, nthreads, out, [&](uint64_t i, uint64_t* b, uint64_t* d) {
        uint64_t s = i * 2 + 12345;
        const uint64_t r = splitmix(s);
        float y, x;
        if (i & 1) {
            y = as_f32((uint32_t)r);
            x = as_f32((uint32_t)(r >> 32));
        } else {
            y = (float)((double)(uint32_t)r / 4294967296.0 * 20.0 - 10.0);
            x = (float)((double)(uint32_t)(r >> 32) / 4294967296.0 * 20.0 - 10.0);
        }
        *b += !same(vslam_kb8::glibc_atan2f(y, x), atan2f(y, x));
        ++*d;
    });
    if (out != stdout) fclose(out);
    return g_failed;
}
