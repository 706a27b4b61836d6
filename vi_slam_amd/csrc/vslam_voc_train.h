/* vslam_voc_train.h -- private: the arithmetic of Vocabulary::create written once for the kernels (vslam_voc_train.hip)
 * and for the host twin (vslam_voc_train_host.cpp), and the host-side tree both of them fill.  The draw functions
 * themselves are in include/vslam_fe.h.  No HIP needed to include this. */
#ifndef VSLAM_VOC_TRAIN_H
#define VSLAM_VOC_TRAIN_H
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vslam_fe.h"

#if defined(__HIPCC__)
#define VT_HD __host__ __device__ __forceinline__
#else
#define VT_HD inline
#endif

/* the in-memory vocabulary file: parsed by vslam_voc_file_open (format 1..3) or trained (format 0) */
struct vslam_voc_file {
    int k = 0, L = 0, scoring = 0, weighting = 0, format = 0, n_words = 0;
    std::vector<int32_t> child_start, child_count, child_ids, word_id;
    std::vector<uint8_t> desc;
    std::vector<double> weight;
};
int vslam_voc_file_fail(int code, const std::string& what); /* sets vslam_voc_file_last_error; returns code */

namespace vslam_vt {

constexpr int kMaxK = 64;
constexpr int kDefaultMaxIter = 10000;
constexpr int kZeroDrawLimit = 64;

/* DescManip::distance for CV_8U (DescManip.cpp:92-119) over 8 dwords */
VT_HD uint32_t hamming(const uint32_t* a, const uint32_t* b) {
    uint32_t d = 0;
    for (int w = 0; w < 8; w++) {
#if defined(__HIP_DEVICE_COMPILE__)
        d += __popc(a[w] ^ b[w]);
#else
        d += (uint32_t)__builtin_popcount(a[w] ^ b[w]);
#endif
    }
    return d;
}

/* (double(rand()) / double(RAND_MAX)) * dist_sum (Vocabulary.cpp:468): two roundings */
VT_HD double cut_of(uint32_t r, uint64_t dist_sum) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(__ddiv_rn((double)r, 2147483647.0), (double)dist_sum);
#else
    return ((double)r / 2147483647.0) * (double)dist_sum; /* built with -ffp-contract=off */
#endif
}

/* the do { cut_d = ... } while (cut_d == 0.0) loop (:464-469) for dist_sum > 0: cut_d is zero exactly when the draw is.
 * *j is the node's draw counter, *redraws counts the zero draws. */
VT_HD double next_cut(uint64_t key, uint32_t* j, uint32_t mask, uint64_t dist_sum, uint32_t* redraws) {
    uint32_t r = 0;
    for (int zeros = 0;;) {
        r = vslamvoc_draw(key, (*j)++, mask);
        if (r != 0) break;
        ++*redraws;
        if (++zeros == kZeroDrawLimit) {
            r = 1;
            break;
        }
    }
    return cut_of(r, dist_sum);
}

/* DescManip::meanValue's threshold (DescManip.cpp:63): a bit is set iff its count >= n / 2 + n % 2.  A group of one
 * copies its feature by the same rule. */
VT_HD uint32_t majority_threshold(uint32_t n) { return n / 2 + n % 2; }

/* ---- host side: the tree in the order the levels produce it, and what turns it into a vslam_voc_file */
struct TreeNode {
    int parent = -1;
    int level = 0;             /* root 0 */
    std::vector<int> children; /* cluster order */
    uint8_t desc[32] = {0};
};

int check_params(const vslam_voc_train_params* p, const int64_t* doc_offsets, int n_docs, vslam_voc_train_params* eff,
                 int64_t* n_features);
/* renumber `tree` (parents before children, root first) into DBoW3's node order, createWords; weights all zero */
vslam_voc_file* finish_tree(const vslam_voc_train_params& p, const std::vector<TreeNode>& tree, vslam_voc_train_stats* st);
/* setNodeWeights (:520-571) from the word of every training feature */
void set_weights(vslam_voc_file& f, const int32_t* word_of_feature, const int64_t* doc_offsets, int n_docs);

}  // namespace vslam_vt
#endif
