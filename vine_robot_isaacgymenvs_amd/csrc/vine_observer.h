// vine_observer.h — what the observers of a step (vine_render.hip, vine_record.hip, vine_episodes.hip, vine_sysid.hip) need of a
// VineHandle (defined in vine_hip.hip), and what each of their launch functions does around its kernel.  Not part of the C ABI: the functions are hidden symbols of libvine_hip.so.
#ifndef VINE_OBSERVER_H
#define VINE_OBSERVER_H

#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/vine.h"

struct VineHandleInfo {
    float* state;                          // SoA block, VF_COUNT * n floats
    const unsigned long long* counters;    // [0] step-count base, [1] finished workgroups of step launches (vine_steps_completed)
    int glog;                              // log2 of the step launch's grid
    int n, device, max_len;
    unsigned flags;
    float L, z1, s0, c0;                   // link_length, joint1_z, sin / cos of phi0
    float soft_limit, success_dist;
    const float* env_params;               // the bound per-env parameter table [VP_COUNT][n] (include/vine_env_params.h) or NULL
    int delay;                             // the configuration's ACTION_DELAY
    float clip_act, rail_scale, fpam_span, fpam_min;      // the constants of task_new_command (vine_task_shared.h)
};

extern "C" {
__attribute__((visibility("hidden"))) int vine_handle_info(VineHandle* h, VineHandleInfo* out);
__attribute__((visibility("hidden"))) const float* vine_reward_matrix_of(VineHandle* h);   // the bound [N,13] matrix, or NULL
__attribute__((visibility("hidden"))) void vine_set_error(const char* msg);    // sets vine_last_error()'s thread-local text
// the tables bound to a handle (NULL where none is) and the global id of its env 0
__attribute__((visibility("hidden"))) int vine_env_tables_of(VineHandle* h, const float** params, const float** inertia,
                                                             unsigned* env_id_offset);
}

// The steps completed, from the handle's counter pair (vine_hip.hip step_of says why it has this form): what the step kernels
// key their random streams by, what every observer kernel schedules itself by, and what vine_get_step_count returns.
__host__ __device__ inline unsigned long long vine_steps_completed(const unsigned long long* counters, int glog) {
    return counters[0] + (counters[1] >> glog);
}

// What every observer's launch function does around its kernel, stated once.
inline int vine_invalid_arg(const char* msg) {
    vine_set_error(msg);
    return VINE_ERR_INVALID_ARG;
}
struct VineDeviceScope {      // the handle's device for the launch, the caller's afterwards
    int prev = -1, dev;
    bool ok = true;
    explicit VineDeviceScope(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
        if (!ok) vine_set_error("hipSetDevice failed");
    }
    ~VineDeviceScope() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};
inline int vine_launch_status(const char* what) {      // hipGetLastError behind a launch, as a VineStatus
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return VINE_OK;
    char msg[200];
    snprintf(msg, sizeof msg, "%s launch: %s", what, hipGetErrorString(e));
    vine_set_error(msg);
    return VINE_ERR_DEVICE;
}

#endif
