// vine_render_internal.h — what vine_render.hip (and the other observers of a step: vine_record.hip, vine_episodes.hip)
// needs of a VineHandle (defined in vine_hip.hip).  Not part of the C ABI: the functions are hidden symbols of libvine_hip.so.
#ifndef VINE_RENDER_INTERNAL_H
#define VINE_RENDER_INTERNAL_H

#include "../../include/vine.h"

struct VineRenderInfo {
    float* state;                          // SoA block, VF_COUNT * n floats
    const unsigned long long* counters;    // [0] step-count base, [1] finished workgroups of step launches (vine_hip.hip step_of)
    int glog;                              // log2 of the step launch's grid
    int n, device, max_len;
    unsigned flags;
    float L, z1, s0, c0;                   // link_length, joint1_z, sin / cos of phi0
    float soft_limit, success_dist;
};

extern "C" {
__attribute__((visibility("hidden"))) int vine_render_info(VineHandle* h, VineRenderInfo* out);
__attribute__((visibility("hidden"))) const float* vine_reward_matrix_of(VineHandle* h);   // the bound [N,13] matrix, or NULL
__attribute__((visibility("hidden"))) void vine_set_error(const char* msg);    // sets vine_last_error()'s thread-local text
}

#endif
