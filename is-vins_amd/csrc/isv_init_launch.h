// isv_init_launch.h -- the host side the batched stages share: the three initialisation stages on a backend handle
// (isv_initial.hip, isv_sfm.hip, isv_relpose.hip), the loop-closure verification (isv_loop.hip), the loop detection
// (isv_bow.hip), the keyframe extraction (isv_keyframe.hip) and the feature tracking (isv_tracker.hip), each of the four on its
// own handle.  (The feature detection, isv_detect.hip, runs on a tracker handle's stream and takes the argument checks from here;
// its five timed sections need more events than run() has.)
// A stage call packs its problems into one pageable upload block, launches one workgroup per problem on the caller's stream and
// copies its outputs back, synchronously.  A stage file keeps what is its own: its header record and problem checks, the packing,
// the kernel launch(es) and the post-processing of the outputs.
#pragma once
#include <chrono>
#include <initializer_list>
#include <string>
#include <vector>
#include "isv_backend_impl.h"

struct InitCopy { void *dst; size_t off, bytes; };   // a device-to-host copy out of the block (skipped when dst is null)

// what a stage call needs of the handle it runs on: its device and stream, the stage's slot (block, events, times) and the
// handle's error string.  `err` is null for a null handle: enter() refuses it.
struct InitCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    InitSlot *slot = nullptr;
    std::string *err = nullptr;
};
inline InitCtx init_ctx(isv_backend *h, int stage) {
    return h ? InitCtx{h->device, h->stream, &h->init_slot[stage], &h->err} : InitCtx{};
}

struct InitCall {
    InitCtx c;
    const char *entry;            // the entry point's name, for the error text
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();

    // the argument checks: ISV_OK to go on, with the handle's device selected when there is work (n > 0)
    template <typename P>
    int enter(int32_t n, const P *const *problems, const void *results) {
        if (!c.err) return ISV_ERR_INVALID_ARG;
        if (n < 0 || (n > 0 && (!problems || !results))) return fail(ISV_ERR_INVALID_ARG, "bad arguments");
        for (int i = 0; i < n; i++)
            if (!problems[i]) return fail(ISV_ERR_INVALID_ARG, "null problem");
        if (n > 0)
            if (const hipError_t e = hipSetDevice(c.device); e != hipSuccess) return hip_fail("hipSetDevice(h->device)", e);
        return ISV_OK;
    }

    int fail(int rc, const char *what) {
        *c.err = std::string(entry) + ": " + what;
        return rc;
    }
    // a failed set-up call: "<call>: <HIP error>", the text HIPCHK leaves
    int hip_fail(const char *call, hipError_t e) {
        *c.err = std::string(call) + ": " + hipGetErrorString(e);
        return ISV_ERR_DEVICE;
    }

    // the device half: grow the slot's block to `bytes`, upload `up` to its start, zero [up.size(), clear_end) (the outputs a
    // refused problem leaves unwritten), launch(block, between) between the kernel events, copy `down` back and synchronise; then
    // post() and the call's times.  A launch of two kernels calls between() between them: it records the slot's middle event, and
    // the slot then also holds each kernel's time.  A failure leaves "<entry>: <HIP error>" and the previous call's times.
    template <typename Launch, typename Post>
    int run(const std::vector<char> &up, size_t clear_end, size_t bytes, Launch launch, std::initializer_list<InitCopy> down, Post post) {
        InitSlot &s = *c.slot;
        hipError_t e = hipSuccess;
        if (bytes > s.cap) {
            if (s.d) (void)hipFree(s.d);
            s.d = nullptr; s.cap = 0;
            if (e = hipMalloc(&s.d, bytes); e != hipSuccess) return hip_fail("hipMalloc(&s.d, bytes)", e);
            s.cap = bytes;
        }
        for (auto &ev : s.ev)
            if (!ev)
                if (e = hipEventCreate(&ev); e != hipSuccess) return hip_fail("hipEventCreate(&e)", e);
        char *d = (char *)s.d;
        bool split = false;
        hipError_t e_mid = hipSuccess;
        auto between = [&] { split = true; e_mid = hipEventRecord(s.ev[2], c.stream); };
        e = hipMemcpyAsync(d, up.data(), up.size(), hipMemcpyHostToDevice, c.stream);
        if (e == hipSuccess) e = hipMemsetAsync(d + up.size(), 0, clear_end - up.size(), c.stream);
        if (e == hipSuccess) e = hipEventRecord(s.ev[0], c.stream);
        if (e == hipSuccess) {
            launch(d, between);
            e = hipGetLastError();
            if (e == hipSuccess) e = e_mid;
        }
        if (e == hipSuccess) e = hipEventRecord(s.ev[1], c.stream);
        for (const InitCopy &cp : down)
            if (e == hipSuccess && cp.dst) e = hipMemcpyAsync(cp.dst, d + cp.off, cp.bytes, hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        float kms = 0.f, k1 = 0.f, k2 = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&kms, s.ev[0], s.ev[1]);
        if (e == hipSuccess && split) e = hipEventElapsedTime(&k1, s.ev[0], s.ev[2]);
        if (e == hipSuccess && split) e = hipEventElapsedTime(&k2, s.ev[2], s.ev[1]);
        if (e != hipSuccess) return fail(ISV_ERR_DEVICE, hipGetErrorString(e));
        post();
        s.kernel_ms = kms; s.part_ms[0] = k1; s.part_ms[1] = k2;
        s.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        return ISV_OK;
    }
};

// isv_internal_*_last_ms: (whole call, kernel) milliseconds of the stage's last successful call on the handle
inline int init_last_ms(isv_backend *h, int stage, double out_ms[2]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->init_slot[stage].call_ms; out_ms[1] = h->init_slot[stage].kernel_ms;
    return ISV_OK;
}
