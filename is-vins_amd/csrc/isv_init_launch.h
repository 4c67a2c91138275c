// isv_init_launch.h -- the host side the batched initialisation stages share (isv_initial.hip, isv_sfm.hip, isv_relpose.hip).
// A stage call packs its problems into one pageable upload block, launches one workgroup per problem on the handle's stream and
// copies its outputs back, synchronously.  A stage file keeps what is its own: its header record and problem checks, the packing,
// the kernel launch and the post-processing of the outputs.
#pragma once
#include <chrono>
#include <initializer_list>
#include <string>
#include <vector>
#include "isv_backend_impl.h"

struct InitCopy { void *dst; size_t off, bytes; };   // a device-to-host copy out of the block (skipped when dst is null)

struct InitCall {
    isv_backend *h;
    int stage;                    // ISV_INIT_*: the handle's slot
    const char *entry;            // the entry point's name, for the error text
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();

    // the argument checks: ISV_OK to go on, with the handle's device selected when there is work (n > 0)
    template <typename P>
    int enter(int32_t n, const P *const *problems, const void *results) {
        if (!h) return ISV_ERR_INVALID_ARG;
        if (n < 0 || (n > 0 && (!problems || !results))) return fail(ISV_ERR_INVALID_ARG, "bad arguments");
        for (int i = 0; i < n; i++)
            if (!problems[i]) return fail(ISV_ERR_INVALID_ARG, "null problem");
        if (n > 0) HIPCHK(h, hipSetDevice(h->device));
        return ISV_OK;
    }

    int fail(int rc, const char *what) {
        h->err = std::string(entry) + ": " + what;
        return rc;
    }

    // the device half: grow the slot's block to `bytes`, upload `up` to its start, zero [up.size(), clear_end) (the outputs a
    // refused problem leaves unwritten), launch(block) between the kernel events, copy `down` back and synchronise; then post()
    // and the call's times.  A failure leaves "<entry>: <HIP error>" and the previous call's times.
    template <typename Launch, typename Post>
    int run(const std::vector<char> &up, size_t clear_end, size_t bytes, Launch launch, std::initializer_list<InitCopy> down, Post post) {
        InitSlot &s = h->init_slot[stage];
        if (bytes > s.cap) {
            if (s.d) (void)hipFree(s.d);
            s.d = nullptr; s.cap = 0;
            HIPCHK(h, hipMalloc(&s.d, bytes));
            s.cap = bytes;
        }
        for (auto &e : s.ev) if (!e) HIPCHK(h, hipEventCreate(&e));
        char *d = (char *)s.d;
        hipError_t e = hipMemcpyAsync(d, up.data(), up.size(), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d + up.size(), 0, clear_end - up.size(), h->stream);
        if (e == hipSuccess) e = hipEventRecord(s.ev[0], h->stream);
        if (e == hipSuccess) {
            launch(d);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(s.ev[1], h->stream);
        for (const InitCopy &c : down)
            if (e == hipSuccess && c.dst) e = hipMemcpyAsync(c.dst, d + c.off, c.bytes, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        float kms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&kms, s.ev[0], s.ev[1]);
        if (e != hipSuccess) return fail(ISV_ERR_DEVICE, hipGetErrorString(e));
        post();
        s.kernel_ms = kms;
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
