// isv_stage_launch.h -- the host side every batched stage shares: the three initialisation stages on a backend handle
// (isv_initial.hip, isv_sfm.hip, isv_relpose.hip), the loop-closure verification (isv_loop.hip), the loop detection
// (isv_bow.hip), the keyframe extraction (isv_keyframe.hip) and the feature tracking (isv_tracker.hip), each of the four on its
// own handle (StageHandle), as are the camera-IMU rotation calibration (isv_exrot.hip) and the IMU pre-integration (isv_preint.hip), and the feature detection (isv_detect.hip), the CLAHE (isv_equalize.hip) and the outlier rejection
// (isv_reject.hip) on a tracker handle's device and stream.
// A stage call packs its problems into one pageable upload block, launches its kernels on the context's stream and copies its
// outputs back, synchronously; the launcher owns the events around and between the kernels and the times read from them.  A stage
// file keeps what is its own: its header record and problem checks, the packing, the kernel launch(es) with their marks and the
// post-processing of the outputs.
#pragma once
#include <chrono>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>
#include "isv_backend_impl.h"

struct StageFill { size_t begin, end; int value = 0; };   // bytes [begin, end) of the block, set before the kernels
struct StageCopy { void *dst; size_t off, bytes; };   // a device-to-host copy out of the block (skipped when dst is null)

// what a stage call needs of the handle it runs on: its device and stream, the stage's slot (block, events, times) and the
// handle's error string.  `err` is null for a null handle: enter() refuses it.
struct StageCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    StageSlot *slot = nullptr;
    std::string *err = nullptr;
};
inline StageCtx init_ctx(isv_backend *h, int stage) {
    return h ? StageCtx{h->device, h->stream, &h->init_slot[stage], &h->err} : StageCtx{};
}

// what a stage's own handle holds for its calls: the current device at creation, a stream of its own, the slot, the error string
struct StageHandle {
    std::string err;
    int device = 0;
    hipStream_t stream = nullptr;
    StageSlot slot;               // the call's device block (grow-only), events and times
    StageCtx ctx() { return StageCtx{device, stream, &slot, &err}; }
    hipError_t open() {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e == hipSuccess && ndev <= 0) e = hipErrorNoDevice;
        if (e == hipSuccess) e = hipGetDevice(&device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        return e;
    }
    void close() {                // (leaves the handle's device selected, for what the owner frees next)
        (void)hipSetDevice(device);
        stage_slot_free(slot);
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};
// the end of a *_create's device set-up: true when it failed, with the reason on stderr (there is no handle to ask yet)
static inline bool stage_open_failed(const char *entry, hipError_t e) {
    if (e == hipSuccess) return false;
    fprintf(stderr, "%s: %s\n", entry, hipGetErrorString(e));
    (void)hipGetLastError();
    return true;
}

struct StageCall {
    StageCtx c;
    const char *entry;            // the entry point's name, for the error text
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    bool time_download = false;   // record `end` behind the downloads, for download_ms: the marker adds some 20 us to a call

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

    // the device half: grow the slot's block to `bytes`; record `begin`, upload `up` to the block's start, set the `fills` (the
    // outputs a refused problem leaves unwritten, zeroed), record `k0`; launch(block, mark); record `k1`, copy `down` back, record
    // `end` (with time_download) and synchronise; then post() and the call's times.  The launch calls mark() at each boundary between its timed sections,
    // at most kStageMarks times and also on a path that launched nothing: the slot then holds each section's time, from k0 through
    // the marks to k1.  post() may enqueue and await more downloads; it returns their error.  A failure -- of a HIP call, of a
    // mark's record, of post() -- leaves "<entry>: <HIP error>" and the previous call's times.
    template <typename Launch, typename Post>
    int run(const std::vector<char> &up, std::initializer_list<StageFill> fills, size_t bytes, Launch launch,
            std::initializer_list<StageCopy> down, Post post) {
        StageSlot &s = *c.slot;
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
        // the kernel sections' boundaries, in s.ev: k0, the marks, k1
        int n_marks = 0;
        hipError_t e_mark = hipSuccess;
        auto mark = [&] {
            if (e_mark != hipSuccess) return;
            if (n_marks == kStageMarks) { e_mark = hipErrorInvalidValue; return; }
            e_mark = hipEventRecord(s.ev[SE_K0 + 1 + n_marks++], c.stream);
        };
        e = hipEventRecord(s.ev[SE_BEGIN], c.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d, up.data(), up.size(), hipMemcpyHostToDevice, c.stream);
        for (const StageFill &f : fills)
            if (e == hipSuccess) e = hipMemsetAsync(d + f.begin, f.value, f.end - f.begin, c.stream);
        if (e == hipSuccess) e = hipEventRecord(s.ev[SE_K0], c.stream);
        if (e == hipSuccess) {
            launch(d, mark);
            e = hipGetLastError();
            if (e == hipSuccess) e = e_mark;
        }
        const int k1 = SE_K0 + 1 + n_marks;
        if (e == hipSuccess) e = hipEventRecord(s.ev[k1], c.stream);
        for (const StageCopy &cp : down)
            if (e == hipSuccess && cp.dst) e = hipMemcpyAsync(cp.dst, d + cp.off, cp.bytes, hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess && time_download) e = hipEventRecord(s.ev[SE_END], c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        float up_ms = 0.f, kms = 0.f, down_ms = 0.f, part[kStageMarks + 1] = {};
        if (e == hipSuccess) e = hipEventElapsedTime(&up_ms, s.ev[SE_BEGIN], s.ev[SE_K0]);
        if (e == hipSuccess) e = hipEventElapsedTime(&kms, s.ev[SE_K0], s.ev[k1]);
        if (e == hipSuccess && time_download) e = hipEventElapsedTime(&down_ms, s.ev[k1], s.ev[SE_END]);
        for (int i = 0; i <= n_marks; i++)
            if (e == hipSuccess) e = hipEventElapsedTime(&part[i], s.ev[SE_K0 + i], s.ev[SE_K0 + i + 1]);
        if (e == hipSuccess) e = post();
        if (e != hipSuccess) return fail(ISV_ERR_DEVICE, hipGetErrorString(e));
        s.upload_ms = up_ms; s.kernel_ms = kms; s.download_ms = down_ms;
        for (int i = 0; i <= kStageMarks; i++) s.part_ms[i] = part[i];
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
