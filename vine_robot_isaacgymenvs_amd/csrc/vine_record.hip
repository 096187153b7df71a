// vine_record.hip — the trajectory recorder (RECORD_TRAJECTORIES) for MI355X (gfx950): include/vine_record.h.
//
// One launch of one wave covers every recorded env: lane k owns env envs[k] (K <= 64).  It gathers the copied fields of
// the SoA state block (st[f * n + e]) and the step's outputs, evaluates the tip's forward kinematics from the joint state
// it has just read (tip_fk_joint of vine_task_shared.h, the same fp32 sequence as tip_fk of vine_hip.hip: the state block's
// tip fields are not stored without introspection), and writes its row of 32 floats as eight 16-byte stores.  Lane 0 also writes the step index.
//
// The scheduled form reads the step counter of the handle (vine_observer.h vine_steps_completed: two 8-byte loads, uniform, so they are
// scalar loads) and returns at once outside a recording window: no other load and no store on that path.
// No atomics; plain C++ stores only.

#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/vine_record.h"
#include "vine_observer.h"
#include "vine_task_shared.h"

namespace {

constexpr int THREADS = 64;      // one wave: VINE_RECORD_MAX_ENVS lanes
static_assert(VINE_RECORD_MAX_ENVS <= THREADS, "one lane per recorded env");
static_assert(VINE_RECORD_FIELDS % 4 == 0, "rows are written as float4");

struct RecordParams {
    int K, num_steps, record_every, slot;      // slot: the explicit form only
    int n, glog;
    unsigned flags;
    float L, z1, s0, c0;
};

template <bool SCHEDULED>
__global__ __launch_bounds__(THREADS) void vine_record_kernel(const RecordParams R, const float* __restrict__ st,
                                                              const unsigned long long* __restrict__ counters,
                                                              const int* __restrict__ envs, const float* __restrict__ actions,
                                                              const float* __restrict__ rew, const long long* __restrict__ reset,
                                                              const long long* __restrict__ progress,
                                                              const unsigned char* __restrict__ timeouts,
                                                              float* __restrict__ ring, long long* __restrict__ steps) {
    const unsigned long long c = vine_steps_completed(counters, R.glog);
    int slot = R.slot;
    if (SCHEDULED) {
        if (c == 0ull) return;
        const unsigned long long m = (c - 1ull) % (unsigned long long)R.record_every;
        if (m >= (unsigned long long)R.num_steps) return;
        slot = (int)m;
    }
    const int k = threadIdx.x;
    if (k == 0) steps[slot] = (long long)c - 1ll;
    if (k >= R.K) return;
    const int n = R.n, e = envs[k];
    float row[VINE_RECORD_FIELDS];
#pragma unroll
    for (int f = 0; f < VINE_RECORD_FIELDS; ++f) row[f] = 0.0f;
    if (e >= 0 && e < n) {
#pragma unroll
        for (int f = 0; f < 2 * VINE_NUM_DOFS; ++f) row[VRF_Q0 + f] = st[(VF_Q0 + f) * n + e];      // q, qd: VF_Q0 .. VF_QD0 + 5
        {   // the tip's forward kinematics of the recorded joint state (vine_task_shared.h)
            float tip[4];
            tip_fk_joint(&row[VRF_Q0], &row[VRF_QD0], R.L, R.z1, R.s0, R.c0, tip);
            row[VRF_TIP_Y] = tip[0]; row[VRF_TIP_Z] = tip[1]; row[VRF_TIP_VY] = tip[2]; row[VRF_TIP_VZ] = tip[3];
        }
        row[VRF_TARGET_Y] = st[VF_TARGET_Y * n + e];
        row[VRF_TARGET_Z] = st[VF_TARGET_Z * n + e];
        row[VRF_ACTION0] = actions[(long long)e * VINE_NUM_ACTIONS];
        row[VRF_ACTION0 + 1] = actions[(long long)e * VINE_NUM_ACTIONS + 1];
        row[VRF_SMOOTHED_U] = st[VF_SMOOTHED_U * n + e];
        row[VRF_REWARD] = rew[e];
        row[VRF_RESET] = reset[e] != 0 ? 1.0f : 0.0f;
        row[VRF_TIMEOUT] = timeouts[e] != 0 ? 1.0f : 0.0f;
        row[VRF_PROGRESS] = (float)progress[e];
        row[VRF_OBJ_DEPTH] = st[VF_OBJ_DEPTH * n + e];
        row[VRF_OBJ_ANGLE] = st[VF_OBJ_ANGLE * n + e];
        if (R.flags & VINE_FLAG_CREATE_SHELF) row[VRF_CONTACT] = st[VF_CONTACT * n + e];
    }
    float4* dst = reinterpret_cast<float4*>(ring + ((long long)slot * R.K + k) * VINE_RECORD_FIELDS);
#pragma unroll
    for (int i = 0; i < VINE_RECORD_FIELDS / 4; ++i) dst[i] = make_float4(row[4 * i], row[4 * i + 1], row[4 * i + 2], row[4 * i + 3]);
}

int validate(const VineRecordConfig* c) {
    if (!c) return vine_invalid_arg("record config is NULL");
    if (c->abi_version != VINE_RECORD_ABI_VERSION) return vine_invalid_arg("VineRecordConfig.abi_version mismatch");
    if (c->num_envs < 1 || c->num_envs > VINE_RECORD_MAX_ENVS) return vine_invalid_arg("record num_envs out of range");
    if (c->num_steps < 1 || c->record_every < c->num_steps) return vine_invalid_arg("need 1 <= num_steps <= record_every");
    return VINE_OK;
}

int launch(VineHandle* h, const VineRecordConfig* cfg, int slot, const int32_t* envs, const float* actions, const float* rew,
           const int64_t* reset, const int64_t* progress, const uint8_t* timeouts, float* ring, int64_t* steps, void* stream,
           bool scheduled) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!h || !envs || !actions || !rew || !reset || !progress || !timeouts || !ring || !steps)
        return vine_invalid_arg("null argument to vine_record");
    if (!scheduled && (slot < 0 || slot >= cfg->num_steps)) return vine_invalid_arg("record slot out of range");
    if (reinterpret_cast<uintptr_t>(ring) & 15u) return vine_invalid_arg("record ring must be 16-byte aligned");
    VineHandleInfo info;
    rc = vine_handle_info(h, &info);
    if (rc) return rc;
    RecordParams R;
    R.K = cfg->num_envs; R.num_steps = cfg->num_steps; R.record_every = cfg->record_every; R.slot = scheduled ? 0 : slot;
    R.n = info.n; R.glog = info.glog; R.flags = info.flags;
    R.L = info.L; R.z1 = info.z1; R.s0 = info.s0; R.c0 = info.c0;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (scheduled)
        hipLaunchKernelGGL(vine_record_kernel<true>, dim3(1), dim3(THREADS), 0, s, R, info.state, info.counters,
                           (const int*)envs, actions, rew, (const long long*)reset, (const long long*)progress, timeouts, ring,
                           (long long*)steps);
    else
        hipLaunchKernelGGL(vine_record_kernel<false>, dim3(1), dim3(THREADS), 0, s, R, info.state, info.counters,
                           (const int*)envs, actions, rew, (const long long*)reset, (const long long*)progress, timeouts, ring,
                           (long long*)steps);
    return vine_launch_status("vine_record");
}

}  // namespace

extern "C" {

int vine_record_config_default(VineRecordConfig* c) {
    if (!c) return vine_invalid_arg("record config is NULL");
    c->abi_version = VINE_RECORD_ABI_VERSION;
    c->record_every = 1000;
    c->num_steps = 500;
    c->num_envs = 1;
    return VINE_OK;
}

int vine_record_config_size(void) { return (int)sizeof(VineRecordConfig); }

int64_t vine_record_ring_bytes(const VineRecordConfig* c) {
    const int rc = validate(c);
    if (rc) return rc;
    return (int64_t)c->num_steps * c->num_envs * VINE_RECORD_FIELDS * (int64_t)sizeof(float);
}

int vine_record(VineHandle* h, const VineRecordConfig* cfg, int32_t slot, const int32_t* envs, const float* actions,
                const float* rew, const int64_t* reset, const int64_t* progress, const uint8_t* timeouts, float* ring,
                int64_t* steps, void* stream) {
    return launch(h, cfg, slot, envs, actions, rew, reset, progress, timeouts, ring, steps, stream, false);
}

int vine_record_scheduled(VineHandle* h, const VineRecordConfig* cfg, const int32_t* envs, const float* actions,
                          const float* rew, const int64_t* reset, const int64_t* progress, const uint8_t* timeouts,
                          float* ring, int64_t* steps, void* stream) {
    return launch(h, cfg, 0, envs, actions, rew, reset, progress, timeouts, ring, steps, stream, true);
}

}  // extern "C"
