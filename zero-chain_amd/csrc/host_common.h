// Host-side runtime helpers shared by the translation units of libzkamd (zkamd.cpp, verify.cpp):
// error reporting, the per-device stream contexts, device / page-locked buffers, HIP-event profiling.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>
#include <thread>
#include <mutex>
#include <atomic>
#include <system_error>
#include <stdexcept>
#include <exception>
#include <new>
#include <functional>
#if defined(__linux__)
#include <sched.h>
#endif
#include "../../include/zkamd.h"
#include "gpu_rt.h"

namespace zkrt {

inline thread_local std::string g_err;

// Streams and the fork event live in a per-DEVICE context that is created on first use and kept for
// the life of the process: handles on different GPUs never tear down each other's streams, and the
// current device - which HIP keeps per host thread - is selected on every entry (use_device), so a
// handle may be driven from any thread.  g_stream & co. are the calling thread's view of the context
// of the device it selected last.
struct DevCtx {
    hipStream_t stream = nullptr;    // main stream: H pipeline, G1 multiexps, stand-alone entries
    hipStream_t stream2 = nullptr;   // side stream: the G2 multiexp of a chunk runs beside the G1 work
    hipStream_t copy = nullptr;      // staging copies of the next block of a host batch
    hipEvent_t ev_fork = nullptr;
    hipEvent_t ev_join = nullptr;    // the side stream's G1 launch set (the A jobs of a chunk) is done
};
inline std::mutex g_ctx_mu;
inline std::map<int, DevCtx*> g_ctxs;   // key: device * 16 + lane
// A worker thread of a zk_pipeline works in its own LANE: a second set of streams on the same device, so
// that the kernels of two chunks can be in flight at once (the latency- and memory-bound phases of one
// beside the issue-bound phases of the other).
inline thread_local int g_lane = 0;
inline thread_local hipStream_t g_stream = nullptr;
inline thread_local hipStream_t g_stream2 = nullptr;
inline thread_local hipStream_t g_copy_stream = nullptr;
inline thread_local hipEvent_t g_ev_fork = nullptr;
inline thread_local hipEvent_t g_ev_join = nullptr;
inline thread_local int g_device = -1;

inline zk_status fail(zk_status st, const std::string& msg) {
    g_err = msg;
    return st;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ZK_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)
#define ZK_TRY(expr)                \
    do {                            \
        zk_status s_ = (expr);      \
        if (s_ != ZK_OK) return s_; \
    } while (0)

inline zk_status use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ZK_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(ZK_ERR_INVALID_ARGUMENT, "device index out of range");
    HIP_TRY(hipSetDevice(device));   // per host thread: never skipped
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    DevCtx*& c = g_ctxs[device * 16 + g_lane];
    if (!c) {
        DevCtx* fresh = new DevCtx();
        if (hipStreamCreateWithFlags(&fresh->stream, hipStreamDefault) != hipSuccess ||
            hipStreamCreateWithFlags(&fresh->stream2, hipStreamDefault) != hipSuccess ||
            hipStreamCreateWithFlags(&fresh->copy, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreate(&fresh->ev_fork) != hipSuccess || hipEventCreate(&fresh->ev_join) != hipSuccess) {
            delete fresh;
            g_ctxs.erase(device * 16 + g_lane);
            return fail(ZK_ERR_DEVICE, "cannot create the streams of device " + std::to_string(device));
        }
        c = fresh;
    }
    g_stream = c->stream;
    g_stream2 = c->stream2;
    g_copy_stream = c->copy;
    g_ev_fork = c->ev_fork;
    g_ev_join = c->ev_join;
    g_device = device;
    return ZK_OK;
}

// Host threads the library may use for the CPU-side legs (witness calculation, proof encoding):
// zk_set_host_threads() / ZKAMD_HOST_THREADS, default = the cores this process may run on.  With one
// process per GPU on an 8-GPU node every rank must take its share of the cores, not all of them.
inline int g_host_threads = 0;
inline unsigned host_threads(size_t work_items, unsigned cap) {
    long n = g_host_threads;
    if (n <= 0) {
        if (const char* env = getenv("ZKAMD_HOST_THREADS")) n = atol(env);
    }
    if (n <= 0) {
#if defined(__linux__) && !defined(ZK_EMU)
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
#endif
        if (n <= 0) n = (long)std::thread::hardware_concurrency();
    }
    if (n <= 0) n = 1;
    if ((unsigned long)n > cap) n = cap;
    if ((size_t)n > work_items) n = (long)work_items;
    return n > 0 ? (unsigned)n : 1u;
}

// No C++ exception crosses the C ABI (the host on the other side is Rust or C: unwinding into it is undefined): every
// exported entry that returns a zk_status is a function-try-block ending in ZK_ABI_CATCH, and work done on other threads
// hands its exception to the thread that joins it (run_threads, SideThread) or turns it into a status on the spot (guarded).
inline zk_status status_of_exception() noexcept {   // inside a catch block
    zk_status st = ZK_ERR_DEVICE;
    try {
        try {
            throw;
        } catch (const std::bad_alloc&) {
            st = ZK_ERR_OUT_OF_MEMORY;
            g_err = "host allocation failed";
        } catch (const std::length_error&) {
            st = ZK_ERR_OUT_OF_MEMORY;
            g_err = "host allocation failed (size)";
        } catch (const std::exception& e) {
            g_err = std::string("internal: ") + e.what();
        } catch (...) {
            g_err = "internal: unknown exception";
        }
    } catch (...) {
    }
    return st;
}
#define ZK_ABI_CATCH \
    catch (...) { return zkrt::status_of_exception(); }
template <class Fn>
inline zk_status guarded(Fn&& fn) noexcept {
    try {
        return fn();
    } catch (...) {
        return status_of_exception();
    }
}

// work(t) for t = 0 .. nthreads - 1 on host threads; the first exception of a worker is rethrown here after all have joined
template <class Fn>
inline void run_threads(unsigned nthreads, Fn& work) {
    if (nthreads <= 1) {
        work(0);
        return;
    }
    std::exception_ptr first;
    std::mutex first_mu;
    auto body = [&](unsigned t) {
        try {
            work(t);
        } catch (...) {
            std::lock_guard<std::mutex> lk(first_mu);
            if (!first) first = std::current_exception();
        }
    };
    // a thread that cannot be started leaves its share to this thread
    std::vector<std::thread> ths;
    unsigned started = 0;
    try {
        ths.reserve(nthreads);
        for (; started < nthreads; started++) ths.emplace_back(std::ref(body), started);
    } catch (...) {
    }
    for (unsigned t = started; t < nthreads; t++) body(t);
    for (auto& th : ths) th.join();
    if (first) std::rethrow_exception(first);
}

// fn(i0, i1) -> zk_status on contiguous ranges of [0, n), one per host thread (host_threads(n, cap)): for work that keeps buffers
// per thread.  The caller gets the status and the message of the lowest range that failed.
template <class Fn>
inline zk_status for_each_range(size_t n, unsigned cap, Fn&& fn) {
    const unsigned nth = host_threads(n, cap);
    std::vector<zk_status> sts(nth, ZK_OK);
    std::vector<std::string> msgs(nth);
    auto work = [&](unsigned t) {
        if ((sts[t] = fn(n * t / nth, n * (t + 1) / nth)) != ZK_OK) msgs[t] = g_err;
    };
    run_threads(nth, work);
    for (unsigned t = 0; t < nth; t++)
        if (sts[t] != ZK_OK) return fail(sts[t], msgs[t]);
    return ZK_OK;
}
// fn(i) -> zk_status for every i of [0, n) on the same ranges: a thread stops at its first failure, and the caller gets the status
// and the message of the lowest failing index
template <class Fn>
inline zk_status for_each_status(size_t n, unsigned cap, Fn&& fn) {
    return for_each_range(n, cap, [&](size_t i0, size_t i1) -> zk_status {
        for (size_t i = i0; i < i1; i++) ZK_TRY(fn(i));
        return ZK_OK;
    });
}

// one helper thread beside the caller (the staging of the next block of a batch); joined on every path out of the scope
struct SideThread {
    std::thread t;
    std::exception_ptr err;
    template <class Fn>
    void start(Fn fn) {
        t = std::thread([this, fn]() mutable {
            try {
                fn();
            } catch (...) {
                err = std::current_exception();
            }
        });
    }
    void join() {
        if (t.joinable()) t.join();
        if (err) {
            std::exception_ptr e = err;
            err = nullptr;
            std::rethrow_exception(e);
        }
    }
    ~SideThread() {
        if (t.joinable()) t.join();
    }
};

// 32 little-endian bytes -> four 64-bit limbs
inline void load_scalar_le(const uint8_t* b, uint64_t out[4]) {
    for (int i = 0; i < 4; i++) {
        uint64_t w = 0;
        for (int j = 7; j >= 0; j--) w = (w << 8) | b[i * 8 + j];
        out[i] = w;
    }
}

// gen_proof's self-check verifies the proofs this library made a moment ago: the prover hands their AFFINE coordinates over
// (A.x A.y | B.x.c0 B.x.c1 B.y.c0 B.y.c1 | C.x C.y: 96 words = 384 bytes per proof, the host's Montgomery layout, which is
// the verifier kernels' own) and the check skips the two decoders - 1.7 ms of square roots at the head of a 6.9 ms
// verification (profiles/r06s_verify_one_launch_list.txt).  prove_chunk (zkamd.cpp) fills what this points at, if anything.
// A cursor: every chunk the prover finishes on this thread appends its proofs' coordinates and advances it.
constexpr size_t OWN_AFFINE_BYTES = 384;
inline thread_local uint8_t* g_own_affine_sink = nullptr;
struct OwnAffineSink {   // set for the duration of a gen_proof call, cleared on every way out
    explicit OwnAffineSink(uint8_t* p) { g_own_affine_sink = p; }
    ~OwnAffineSink() { g_own_affine_sink = nullptr; }
};

enum VerifyForm { VERIFY_PER_PROOF = 0, VERIFY_COMBINED = 1, VERIFY_AUTO = 2 };   // verify.cpp verify_batch (declared in handles.h)

// Test hooks (fault injection) and debug prints are compiled in only under -DZK_TEST_HOOKS: the emulation build and
// libzkamd_hooks.so, which the three GPU tests that need them load.  The shipped libzkamd.so - a library that handles
// spending keys - reads none of these variables (tests/test_abi.py checks the strings are not in it).
#ifdef ZK_TEST_HOOKS
inline const char* hook_env(const char* name) { return getenv(name); }
#else
inline const char* hook_env(const char*) { return nullptr; }
#endif

// What the library holds and what it wiped (zk_memory_stats): every device and page-locked buffer is zeroed before it is
// returned to the runtime unless it was marked public (the tables of a key: CRS points, twiddles) - the assignment, the
// scalar vectors, the witness kernels' scratch, the digits and bucket sums of a multiexp carry the bits of dec_key,
// randomness and the spending-key-derived values, and a multi-tenant GPU is not a process heap (VERDICT r5 missing 5).
struct MemStats {
    std::atomic<uint64_t> dev_live{0}, dev_freed_secret{0}, dev_wiped{0}, pin_live{0}, pin_freed{0}, pin_wiped{0};
};
inline MemStats g_mem;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool owned = true;
    bool is_public = false;   // nothing secret ever lives here: freed without the wipe
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && owned) {
            if (!is_public) {
                g_mem.dev_freed_secret += cap;
                // whatever still runs on the lanes' streams must not write here after the wipe; at the points a buffer is
                // released (a handle is freed, a workspace regrows between calls) nothing is in flight and this costs microseconds
                (void)hipDeviceSynchronize();
                if (hipMemset(p, 0, cap) == hipSuccess) g_mem.dev_wiped += cap;
            }
            (void)hipFree(p);
            g_mem.dev_live -= cap;
        }
        p = nullptr;
        cap = 0;
    }
    // a read-only view of another buffer (tables shared between the lanes of a pipeline); the owner must outlive it
    void borrow(const DevBuf& o) {
        release();
        p = o.p;
        cap = o.cap;
        owned = false;
    }
    zk_status ensure(size_t bytes) {
        if (bytes <= cap) return ZK_OK;
        if (!owned) return fail(ZK_ERR_INVALID_ARGUMENT, "internal: a borrowed buffer cannot grow");
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            return fail(ZK_ERR_OUT_OF_MEMORY, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
        }
        cap = bytes;
        g_mem.dev_live += cap;
        return ZK_OK;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
    // room for n elements of the host array v, then a blocking copy of them (a std::vector: all of it)
    template <class T>
    zk_status upload(const T* v, size_t n) {
        ZK_TRY(ensure(n * sizeof(T)));
        HIP_TRY(hipMemcpy(p, v, n * sizeof(T), hipMemcpyHostToDevice));
        return ZK_OK;
    }
    template <class T>
    zk_status upload(const std::vector<T>& v) {
        return upload(v.data(), v.size());
    }
};

// page-locked host memory: asynchronous copies into pageable memory block the calling thread until
// the copy has run, which would serialise whatever is enqueued after them on other streams
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() {}
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    void release() {
        if (p) {
            explicit_bzero(p, cap);   // staging of assignments, of (r, s), of results: wiped like the device side
            g_mem.pin_wiped += cap;
            g_mem.pin_freed += cap;
            (void)hipHostFree(p);
            g_mem.pin_live -= cap;
        }
        p = nullptr;
        cap = 0;
    }
    zk_status ensure(size_t bytes) {
        if (bytes <= cap) return ZK_OK;
        release();
        if (hipHostMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            return fail(ZK_ERR_OUT_OF_MEMORY, "hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
        }
        cap = bytes;
        g_mem.pin_live += cap;
        return ZK_OK;
    }
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};

// ------------------------------------------------------------------------------------------
// HIP-event profiling of named kernels (zk_profile_*)
// ------------------------------------------------------------------------------------------
struct ProfRec {
    std::string name;
    hipEvent_t a, b;
};
// process-wide (the GPU thread of a zk_pipeline records into the same list the caller reads)
inline std::mutex g_prof_mu;
inline bool g_prof = false;
inline std::vector<ProfRec> g_recs;

struct ProfScope {
    bool on = false;
    hipStream_t st;
    hipEvent_t end = nullptr;
    ProfScope(const char* name, hipStream_t stream = nullptr) : st(stream ? stream : g_stream) {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_prof) return;
        ProfRec r;
        r.name = name;
        if (hipEventCreate(&r.a) != hipSuccess) return;
        if (hipEventCreate(&r.b) != hipSuccess) {
            (void)hipEventDestroy(r.a);
            return;
        }
        (void)hipEventRecord(r.a, st);
        end = r.b;
        on = true;
        g_recs.push_back(r);
    }
    ~ProfScope() {
        if (on) (void)hipEventRecord(end, st);
    }
};

}  // namespace zkrt
