// vine_env_redraw.hip — a new plant for every episode (ENV_PARAMS_PER_EPISODE) for MI355X (gfx950): include/vine_env_redraw.h.
//
// One lane per env, VINE_ENV_REDRAW_THREADS envs per workgroup, no LDS, no atomics.  A lane whose reset flag is clear loads
// that one word and leaves; a lane whose flag is set hashes (seed, name, global env id, episode) per name of the spec, forms
// its column in float64 and stores it: up to 28 + 31 coalesced 4-byte stores per lane, and 16 more where the delay changed.
//
// THIS TRANSLATION UNIT IS COMPILED WITH -ffp-contract=off (native.py): `a + b * c` must stay a multiply and an add, each
// rounded, as numpy and the host pass form it.  Under the flags of the other translation units hipcc fuses it on gfx950, a
// pragma or __dmul_rn notwithstanding, and a column would differ from utils/env_params.py draw_columns in the last bit.
//
// `redraw_value` and `redraw_column` (vine_env_redraw_draw.h, shared with vine_env_adr.hip) are host and device functions: vine_env_redraw_spec forms the candidates it checks with
// the statements the kernel forms its columns with.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/vine_env_redraw.h"
#include "vine_env_redraw_draw.h"
#include "vine_observer.h"

namespace {

constexpr int THREADS = VINE_ENV_REDRAW_THREADS;

__global__ __launch_bounds__(THREADS) void vine_env_redraw_kernel(const VineEnvRedrawSpec S, const int n, const unsigned env_off,
                                                                  const long long* __restrict__ reset, float* __restrict__ st,
                                                                  float* __restrict__ ptab, float* __restrict__ itab,
                                                                  int* __restrict__ episode_index) {
    const int e = blockIdx.x * THREADS + (int)threadIdx.x;
    if (e >= n) return;
    if (reset[e] == 0) return;
    const int k = episode_index[e] + 1;
    episode_index[e] = k;
    const unsigned long long g = (unsigned long long)env_off + (unsigned long long)e;

    double v[VR_NAMES];
#pragma unroll
    for (int s = 0; s < VR_NAMES; ++s)
        v[s] = S.name[s].form != VINE_REDRAW_ABSENT
                   ? redraw_value(S.name[s], s == VR_ACTION_DELAY, S.values, S.seed, g, (unsigned long long)(long long)k)
                   : 0.0;
    float pcol[VP_COUNT], icol[VI_COUNT];
    redraw_column(S, v, pcol, icol);

    if (S.name[VR_ACTION_DELAY].form != VINE_REDRAW_ABSENT) {
        const float old_delay = ptab[(size_t)VP_ACTION_DELAY * n + e];
        if (old_delay != pcol[VP_ACTION_DELAY]) {
#pragma unroll
            for (int j = 0; j < 2 * VINE_MAX_DELAY; ++j) st[(size_t)(VF_FIFO0 + j) * n + e] = 0.0f;
        }
    }
#pragma unroll
    for (int s = 0; s < VR_FPAM_K; ++s)
        if (S.name[s].form != VINE_REDRAW_ABSENT) ptab[(size_t)s * n + e] = pcol[s];
#pragma unroll
    for (int s = VR_FPAM_K; s <= VR_FPAM_B; ++s)
        if (S.name[s].form != VINE_REDRAW_ABSENT) {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int p = VP_FPAM_K0 + (s - VR_FPAM_K) * NL + j;
                ptab[(size_t)p * n + e] = pcol[p];
            }
        }
    if (itab) {
#pragma unroll
        for (int r = 0; r < VI_COUNT; ++r) itab[(size_t)r * n + e] = icol[r];
    }
}

int bad_name(int s, const char* why) { return named_refusal("env redraw spec", kRedrawNames[s], why); }

// a refusal of the table checks, which saw candidate column i as a table of one env: "of env 0" -> "of candidate i"
int refused_candidate(int rc, int i) {
    std::string msg = vine_last_error();
    const size_t at = msg.find(" of env 0 ");
    if (at != std::string::npos) msg.replace(at, 10, " of candidate " + std::to_string(i) + " ");
    vine_set_error(msg.c_str());
    return rc;
}

}  // namespace

extern "C" {

int vine_env_redraw_spec_size(void) { return (int)sizeof(VineEnvRedrawSpec); }

int vine_env_redraw_spec(const VineConfig* cfg, const VineEnvRedrawName names[VR_NAMES], const double* host_values,
                         const double* device_values, int num_values, VineEnvRedrawSpec* out) {
    if (!cfg || !names || !out) return vine_invalid_arg("null argument to vine_env_redraw_spec");
    if (num_values < 0 || (num_values > 0 && (!host_values || !device_values)))
        return vine_invalid_arg("null argument to vine_env_redraw_spec: the value lists need a host and a device array");
    VineEnvRedrawSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_REDRAW_ABI_VERSION;
    S.num_values = num_values;
    S.seed = cfg->seed;
    S.values = device_values;
    float irow[VI_COUNT];
    int rc = vine_env_params_row(cfg, S.base_params);
    if (rc) return rc;
    rc = vine_env_inertia_row(cfg, irow);
    if (rc) return rc;
    for (int r = 0; r < VI_PRIMARY_COUNT; ++r) S.base_inertia[r] = irow[r];
    S.link_length = cfg->link_length; S.link_com = cfg->link_com; S.gravity = cfg->gravity;
    int width = 1;
    bool any = false;
    for (int s = 0; s < VR_NAMES; ++s) {
        const VineEnvRedrawName& nm = names[s];
        S.name[s] = nm;
        const NamedCheck c = named_check(nm, host_values, num_values, true, any_value);
        if (c.why) return bad_name(s, c.why);
        if (nm.form == VINE_REDRAW_ABSENT) continue;
        any = true;
        if (nm.form == VINE_REDRAW_RANGE) {
            if (s == VR_ACTION_DELAY && (nm.lo != std::floor(nm.lo) || nm.hi != std::floor(nm.hi)))
                return bad_name(s, "an integer parameter takes an integer range");
            if (width < 2) width = 2;
        } else if (nm.form == VINE_REDRAW_VALUES && width < nm.values_count) {
            width = nm.values_count;
        }
    }
    if (!any) return vine_invalid_arg("env redraw spec: no name is present, nothing to redraw");
    // what the spec CAN give an env: candidate column i takes every name's candidate i (mod its count)
    for (int i = 0; i < width; ++i) {
        double v[VR_NAMES];
        for (int s = 0; s < VR_NAMES; ++s) {
            const VineEnvRedrawName& nm = S.name[s];
            v[s] = 0.0;
            if (nm.form == VINE_REDRAW_NUMBER) v[s] = nm.lo;
            else if (nm.form == VINE_REDRAW_RANGE) v[s] = (i & 1) ? nm.hi : nm.lo;
            else if (nm.form == VINE_REDRAW_VALUES) v[s] = host_values[nm.values_first + i % nm.values_count];
        }
        float pcol[VP_COUNT], icol[VI_COUNT];
        redraw_column(S, v, pcol, icol);
        rc = vine_env_params_check(cfg, pcol, 1);
        if (rc) return refused_candidate(rc, i);
        if (names_inertia(S)) {
            rc = vine_env_inertia_check(cfg, icol, 1);
            if (rc) return refused_candidate(rc, i);
        }
    }
    S.checked = 1u;
    *out = S;
    return VINE_OK;
}

int vine_env_redraw_scheduled(VineHandle* h, const VineEnvRedrawSpec* spec, const int64_t* reset, float* params_table,
                              float* inertia_table, int32_t* episode_index, void* stream) {
    if (!h || !spec || !reset || !params_table || !episode_index) return vine_invalid_arg("null argument to vine_env_redraw_scheduled");
    if (spec->abi_version != VINE_ENV_REDRAW_ABI_VERSION) return vine_invalid_arg("VineEnvRedrawSpec.abi_version mismatch");
    if (spec->checked != 1u) return vine_invalid_arg("VineEnvRedrawSpec was not filled by vine_env_redraw_spec");
    if (spec->num_values > 0 && !spec->values) return vine_invalid_arg("VineEnvRedrawSpec.values is NULL");
    VineHandleInfo info;
    int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    const float *bound_params = nullptr, *bound_inertia = nullptr;
    unsigned env_off = 0;
    rc = vine_env_tables_of(h, &bound_params, &bound_inertia, &env_off);
    if (rc) return rc;
    if (!bound_params)
        return vine_invalid_arg("vine_env_redraw_scheduled needs a parameter table bound to the handle (vine_bind_env_params)");
    if (bound_params != params_table)
        return vine_invalid_arg("vine_env_redraw_scheduled: params_table is not the table bound to the handle");
    if (names_inertia(*spec) && (!bound_inertia || !inertia_table))
        return vine_invalid_arg("vine_env_redraw_scheduled: the spec names masses and needs an inertia table bound to the handle "
                                "(vine_bind_env_inertia)");
    if (inertia_table && bound_inertia != inertia_table)
        return vine_invalid_arg("vine_env_redraw_scheduled: inertia_table is not the table bound to the handle");
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const int blocks = (info.n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(vine_env_redraw_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, *spec, info.n, env_off,
                       (const long long*)reset, info.state, params_table, names_inertia(*spec) ? inertia_table : nullptr,
                       episode_index);
    return vine_launch_status("vine_env_redraw");
}

}  // extern "C"
