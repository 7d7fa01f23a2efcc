/* dpx_host.h -- what every host unit of libdpxalign.so shares: the device and the error text of the calling thread, the knob snapshot
 * and the DPX_TRACE phase timer.  dpx_host.cpp holds the state; bind_device is dpx_capi.cpp's (it may have to call dpx_init). */
#ifndef DPX_HOST_H
#define DPX_HOST_H

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <string>

#include "dpx_plan.h" /* (Knobs, align_up; brings dpx_kernels.h, dpx_dir.h, dpx_banddir.h and dpx_layout.h) */

#pragma GCC visibility push(hidden) /* (internal to libdpxalign.so: not part of its ABI) */
namespace dpx_host {

/* (inline, with their initialisers in sight of every unit: an `extern thread_local` makes every other unit call the variable's
 * initialisation function through a weak reference, and a hidden weak reference that stays undefined -- t_device has no such function --
 * does not compare equal to null in position-independent code: the call lands on the library's load address) */
inline thread_local int t_device = -1; /* device of the call this thread is in (a batch's own device, or the default) */
inline thread_local std::string t_err;

int hip_fail(hipError_t e, const char *what);
#define HIP_TRY(call)                                                  \
    do {                                                               \
        hipError_t e__ = (call);                                       \
        if (e__ != hipSuccess) return ::dpx_host::hip_fail(e__, #call); \
    } while (0)

/* Make `device` (-1: the default device, initialising device 0 if dpx_init() was never called) current for this thread.
 * Every buffer / stream cache entry carries its device, so one process can drive several GPUs: a batch lives on the
 * device it was created on and every call on it binds that device first. */
int bind_device(int device = -1);

/* The environment is read in refresh_knobs and nowhere else; the snapshot everything else reads is dpx_plan.h's Knobs. */
void refresh_knobs();
Knobs knobs();

/* DPX_TRACE=1: phase timings of dpx_batch_create / destroy on stderr (development aid) */
struct PhaseTrace {
    bool on = knobs().trace;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[dpx] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

} // namespace dpx_host
#pragma GCC visibility pop
#endif
