/* vslam_mem.h -- private: who owns an allocation.  vslam_buf<T, Space> is a move-only owner of one block of a memory
 * space; its destructor frees, so an object's members are the whole list of what it owns and a destroy function keeps
 * only what has an order (streams, locks).  The generic part includes nothing from HIP (tests/cpp/mem_owner.cpp compiles
 * it alone); the two product spaces, the event owner and HIPCHK follow below it for the .hip files. */
#ifndef VSLAM_MEM_H
#define VSLAM_MEM_H
#include <cstddef>
#include <type_traits>
#include <utility>

#include "../../include/vslam_fe.h"

/* Space supplies   static int alloc(void** p, size_t bytes)   -- VSLAM_OK, or an error code with the thread's error text set
 *                  static void free(void* p, size_t bytes)    -- bytes as given to alloc */
template <class T, class Space>
struct vslam_buf {
    static constexpr size_t kElem = sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type);

    vslam_buf() = default;
    vslam_buf(const vslam_buf&) = delete;
    vslam_buf& operator=(const vslam_buf&) = delete;
    vslam_buf(vslam_buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
        o.p_ = nullptr;
        o.bytes_ = 0;
    }
    vslam_buf& operator=(vslam_buf&& o) noexcept {
        if (this != &o) {
            release();
            swap(o);
        }
        return *this;
    }
    ~vslam_buf() { release(); }

    void swap(vslam_buf& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
    }
    void release() {
        if (p_) Space::free(p_, bytes_);
        p_ = nullptr;
        bytes_ = 0;
    }
    /* a fresh block of `count` elements; what the buffer held is released first.  Empty and size 0 after a failure. */
    int alloc(size_t count) {
        release();
        void* p = nullptr;
        const int rc = Space::alloc(&p, count * kElem);
        if (rc != VSLAM_OK) return rc;
        p_ = (T*)p;
        bytes_ = count * kElem;
        return VSLAM_OK;
    }
    /* grow-only, contents NOT preserved: a smaller request reuses the block of a larger one before it */
    int ensure(size_t count) { return bytes_ >= count * kElem ? VSLAM_OK : alloc(count); }

    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    size_t count() const { return bytes_ / kElem; }
    operator T*() const { return p_; } /* launch sites and pointer arithmetic read as with a raw pointer */
    template <class U>
    explicit operator U*() const { return (U*)p_; } /* ... and so does a cast that carves it: (float*)buf */

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

/* a host table into an allocation of its own (at least 4 bytes, so that an empty table has an address too);
 * Space::upload(dst, src, bytes) copies */
template <class T, class Space>
int vslam_upload(vslam_buf<T, Space>& dst, const void* src, size_t bytes) {
    constexpr size_t E = vslam_buf<T, Space>::kElem;
    const int rc = dst.alloc(((bytes ? bytes : 4) + E - 1) / E);
    if (rc != VSLAM_OK || !bytes) return rc;
    return Space::upload(dst.get(), src, bytes);
}

#if defined(__HIPCC__)
/* ------------------------------------------------------------------ the product's two spaces (HIP) */
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

std::string& vslam_err();
#define g_err (vslam_err())

#define HIPCHK(call)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
            return VSLAM_ERR_HIP;                                                                \
        }                                                                                        \
    } while (0)

int vslam_pinned_alloc(void** p, size_t bytes); /* hipHostMalloc on the device's NUMA node; returns a hipError_t (vslam_upload.hip) */

/* live bytes and live blocks of a space, process-wide (vslam_dbg_live_memory): on a shared device the free-memory figure
 * cannot tell a leak of ours from a neighbour's allocation */
struct vslam_mem_counters {
    std::atomic<unsigned long long> bytes{0}, blocks{0};
    void add(size_t n) {
        bytes += n;
        blocks++;
    }
    void sub(size_t n) {
        bytes -= n;
        blocks--;
    }
};
inline vslam_mem_counters g_vslam_device_mem, g_vslam_pinned_mem;

struct vslam_device_space {
    static int alloc(void** p, size_t bytes) {
        HIPCHK(hipMalloc(p, bytes));
        g_vslam_device_mem.add(bytes);
        return VSLAM_OK;
    }
    static void free(void* p, size_t bytes) {
        (void)hipFree(p);
        g_vslam_device_mem.sub(bytes);
    }
    static int upload(void* dst, const void* src, size_t bytes) {
        HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return VSLAM_OK;
    }
};
struct vslam_pinned_space {
    static int alloc(void** p, size_t bytes) {
        HIPCHK((hipError_t)vslam_pinned_alloc(p, bytes));
        g_vslam_pinned_mem.add(bytes);
        return VSLAM_OK;
    }
    static void free(void* p, size_t bytes) {
        (void)hipHostFree(p);
        g_vslam_pinned_mem.sub(bytes);
    }
};
template <class T>
using vslam_dbuf = vslam_buf<T, vslam_device_space>; /* HBM */
template <class T>
using vslam_hbuf = vslam_buf<T, vslam_pinned_space>; /* pinned host memory */

/* an event created on first use and destroyed with its owner */
struct vslam_event {
    vslam_event() = default;
    vslam_event(const vslam_event&) = delete;
    vslam_event& operator=(const vslam_event&) = delete;
    ~vslam_event() {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    int ensure(unsigned flags = hipEventDefault) {
        if (!ev_) HIPCHK(hipEventCreateWithFlags(&ev_, flags));
        return VSLAM_OK;
    }
    operator hipEvent_t() const { return ev_; }

private:
    hipEvent_t ev_ = nullptr;
};
#endif /* __HIPCC__ */

#endif
