/* vslam_async.h -- private: what sits beside the staging block of an enqueue / wait pair (X_async, X_wait, the blocking X and
 * vslam_fe_get_X_profile): the record of the operation in flight and the HIP-event timer of its kernels' spans.  Included by
 * vslam_ctx.h. */
#ifndef VSLAM_ASYNC_H
#define VSLAM_ASYNC_H
#include <hip/hip_runtime.h>

#include "vslam_mem.h"

/* the members that the compiler does not inline stay out of the library's exported symbols */
#define VSLAM_PRIVATE __attribute__((visibility("hidden")))

/* One enqueue at a time per staging block.  _async: begin() refuses while a search is in flight, then -- the arguments
 * accepted -- set().  _wait: ready() refuses when nothing is enqueued or when the other form of the block was (`kind`, for
 * the one block that serves two: SearchLocalPoints with one camera and with a rig); the wait's own arguments checked, take()
 * returns to idle BEFORE the stream wait, so that a wait that fails leaves the context reusable, and says whether the
 * search was empty: nothing was launched, there is nothing to wait for. */
struct VSLAM_PRIVATE vslam_pending {
    enum State { IDLE, IN_FLIGHT, EMPTY };
    State state = IDLE;
    int kind = 0;
    int n = 0, jobs = 0; /* what _wait sizes its outputs by: match slots (per job), jobs */

    bool in_flight() const { return state == IN_FLIGHT; }
    int begin(const char* in_flight_msg) const {
        if (!in_flight()) return VSLAM_OK;
        g_err = in_flight_msg;
        return VSLAM_ERR_INVALID;
    }
    void set(bool empty, int kind_ = 0) {
        state = empty ? EMPTY : IN_FLIGHT;
        kind = kind_;
    }
    int ready(int kind_ = 0, const char* other_kind_msg = nullptr) const {
        if (state != IDLE && kind == kind_) return VSLAM_OK;
        g_err = state == IDLE ? "nothing enqueued" : other_kind_msg;
        return VSLAM_ERR_INVALID;
    }
    bool take() {
        const bool empty = state == EMPTY;
        state = IDLE;
        return empty;
    }
};

/* K consecutive spans between K + 1 events on a stream, summed over the operations waited for while vslam_fe_set_profiling
 * is on.  _async: arm() before anything is launched, mark(i) between the launches (or event(i) for a launcher that records
 * the middle marks itself); _wait: collect() behind the stream wait.  Not armed, every step is a no-op and event() null. */
template <int K>
struct VSLAM_PRIVATE vslam_span_timer {
    vslam_event ev[K + 1];
    bool armed = false;
    double ms[K] = {};
    long passes = 0;

    int arm(bool profiling) {
        armed = false;
        for (int i = 0; i <= K && profiling; i++)
            if (int rc = ev[i].ensure()) return rc;
        armed = profiling;
        return VSLAM_OK;
    }
    void mark(int i, hipStream_t st) const {
        if (armed) (void)hipEventRecord(ev[i], st);
    }
    hipEvent_t event(int i) const { return armed ? (hipEvent_t)ev[i] : nullptr; }
    int collect() {
        if (!armed) return VSLAM_OK;
        armed = false;
        float t[K];
        for (int i = 0; i < K; i++) HIPCHK(hipEventElapsedTime(&t[i], ev[i], ev[i + 1]));
        for (int i = 0; i < K; i++) ms[i] += t[i];
        passes++;
        return VSLAM_OK;
    }
    void reset() {
        for (int i = 0; i < K; i++) ms[i] = 0;
        passes = 0;
    }
    /* the getters: every sum whose pointer is given, and the count */
    void read(double* const (&out)[K], long* out_passes) const {
        for (int i = 0; i < K; i++)
            if (out[i]) *out[i] = ms[i];
        if (out_passes) *out_passes = passes;
    }
};

#endif
