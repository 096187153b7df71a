// vine_episodes.hip — the per-episode task log (EPISODE_LOG) for MI355X (gfx950): include/vine_episodes.h.
//
// One lane per env, VINE_EPISODES_THREADS envs per workgroup.  Every step a lane reads rew, the reset flag, its four
// accumulators (coalesced: struct of arrays) and two terms of its reward-matrix row (dist, reached), and writes the four
// accumulators back.  That is all an idle step does: the three other terms, the time-out flag and the four state fields are
// loaded by the lanes whose episode ended, and the slot atomic, the reductions and the totals are touched only by a wave
// / workgroup that finished an episode.
//
// The update and finish rules are those of the EVAL block of vine_step_quad_kernel (vine_hip.hip, "episode accounting"):
// that block is the twin of `account` below and the two must change together.  It is not shared through a header because
// the step kernels' register allocation is not to move for an observer.
//
// Totals: the eight count columns of a wave are popcounts of ballots; the four real-valued sums (and the two integer-valued
// ones that are not counts) are reduced in float64 by an xor butterfly, then over the four waves through LDS in a fixed
// order, and added to the workgroup's own row: no float atomics, bit-reproducible.
// Slots: one returning 64-bit integer atomicAdd per wave that finished an episode (the leader adds the popcount, the wave
// reads the base back by a shuffle); a lane's rank is the popcount of the ballot below it.  With capacity < N the launch
// is ONE workgroup (SERIAL) that walks the chunks in order and hands out slots itself: no atomic, env order, and rows the
// same step would lap are skipped, so no two waves ever write one slot.

#include <hip/hip_runtime.h>

#include "../../include/vine_episodes.h"
#include "vine_observer.h"

namespace {

constexpr int THREADS = VINE_EPISODES_THREADS;
constexpr int WAVES = THREADS / 64;
static_assert(WAVES == 4, "the workgroup's sums are folded as (w0 + w1) + (w2 + w3)");
static_assert(VINE_EPISODES_WORDS == 16, "rows are written as four 16-byte stores");
static_assert(VINE_EVAL_EPISODE_FIELDS == 4 && VINE_EVAL_NUM_TOTALS == 12, "the accounting of vine_step_eval");

struct EpisodesParams {
    int n, glog, nchunks;
    unsigned flags;
    long long capacity;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ int popc_below(unsigned long long ballot, int lane) {
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

template <bool SERIAL>
__global__ __launch_bounds__(THREADS) void vine_episodes_kernel(const EpisodesParams E, const float* __restrict__ st,
                                                                const unsigned long long* __restrict__ counters,
                                                                const float* __restrict__ rmat, const float* __restrict__ rew,
                                                                const long long* __restrict__ reset,
                                                                const unsigned char* __restrict__ timeouts,
                                                                float* __restrict__ episode, double* __restrict__ totals,
                                                                unsigned* __restrict__ table,
                                                                unsigned long long* __restrict__ cursor) {
    const unsigned long long c = vine_steps_completed(counters, E.glog);
    if (c == 0ull) return;
    const int end_step = (int)(c - 1ull);
    const int n = E.n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double red[WAVES][VINE_EVAL_NUM_TOTALS];
    __shared__ int wave_rows[WAVES];

    // SERIAL: the rows this step appends, the first of them that survives the step's own lap, the cursor before the step
    long long step_rows = 0, first_kept = 0, run = 0;
    unsigned long long base0 = 0ull;
    if (SERIAL && table) {
        for (int chunk = 0; chunk < E.nchunks; ++chunk) {
            const int e = chunk * THREADS + (int)threadIdx.x;
            step_rows += __syncthreads_count(e < n && reset[e] != 0);
        }
        first_kept = step_rows > E.capacity ? step_rows - E.capacity : 0;
        base0 = cursor[0];
    }

    for (int chunk = blockIdx.x; chunk < E.nchunks; chunk += gridDim.x) {
        const int e = chunk * THREADS + (int)threadIdx.x;
        const bool valid = e < n;
        bool done = false, reached = false;
        float er = 0.0f, el = 0.0f, emin = 0.0f, efirst = 0.0f, dist = 0.0f;
        if (valid) {
            // ---- account: the twin of vine_step_quad_kernel's EVAL block
            const float* rm = rmat + (size_t)e * VINE_NUM_REWARDS;
            dist = -rm[0];
            reached = rm[2] != 0.0f;
            done = reset[e] != 0;
            er = episode[(size_t)VINE_EVAL_EP_RETURN * n + e] + rew[e];
            el = episode[(size_t)VINE_EVAL_EP_LENGTH * n + e] + 1.0f;
            emin = fminf(episode[(size_t)VINE_EVAL_EP_MIN_DIST * n + e], dist);
            const float first = episode[(size_t)VINE_EVAL_EP_FIRST_REACH * n + e];
            efirst = (first == 0.0f && reached) ? el : first;
            episode[(size_t)VINE_EVAL_EP_RETURN * n + e] = done ? 0.0f : er;
            episode[(size_t)VINE_EVAL_EP_LENGTH * n + e] = done ? 0.0f : el;
            episode[(size_t)VINE_EVAL_EP_MIN_DIST * n + e] = done ? __builtin_huge_valf() : emin;
            episode[(size_t)VINE_EVAL_EP_FIRST_REACH * n + e] = done ? 0.0f : efirst;
        }
        if (!__syncthreads_or(done)) continue;      // nobody in this workgroup finished (uniform): nothing else is touched

        bool to = false, limit_hit = false, tip_limit = false, contact = false;
        if (done) {
            const float* rm = rmat + (size_t)e * VINE_NUM_REWARDS;
            to = timeouts[e] != 0;
            limit_hit = rm[9] != 0.0f;
            tip_limit = rm[11] != 0.0f && (E.flags & VINE_FLAG_USE_TIP_LIMIT_HIT_RESET);
            contact = rm[12] < 0.0f && (E.flags & VINE_FLAG_USE_NONZERO_CONTACT_FORCE_RESET);
        }
        const unsigned long long b_done = __ballot(done);

        // ---- the ring
        if (table) {
            const int rows = __popcll(b_done);
            long long k = -1;
            if (SERIAL) {
                if (lane == 0) wave_rows[wave] = rows;
                __syncthreads();
                long long before = run;
                for (int w = 0; w < wave; ++w) before += wave_rows[w];
                const long long j = before + popc_below(b_done, lane);
                if (done && j >= first_kept) k = (long long)base0 + j;
                run += (wave_rows[0] + wave_rows[1]) + (wave_rows[2] + wave_rows[3]);
            } else if (rows) {
                unsigned long long base = 0ull;
                if (lane == __ffsll((long long)b_done) - 1) base = atomicAdd(cursor, (unsigned long long)rows);
                base = __shfl(base, __ffsll((long long)b_done) - 1);
                if (done) k = (long long)(base + (unsigned long long)popc_below(b_done, lane));
            }
            if (k >= 0) {
                const unsigned reason = (to ? VINE_EPISODES_END_TIMEOUT : 0u) | (limit_hit ? VINE_EPISODES_END_RAIL_LIMIT : 0u) |
                                        (tip_limit ? VINE_EPISODES_END_TIP_LIMIT : 0u) | (contact ? VINE_EPISODES_END_CONTACT : 0u);
                uint4* dst = reinterpret_cast<uint4*>(table + (size_t)(k % E.capacity) * VINE_EPISODES_WORDS);
                dst[0] = make_uint4((unsigned)e, (unsigned)end_step, __float_as_uint(el), __float_as_uint(er));
                dst[1] = make_uint4(__float_as_uint(efirst != 0.0f ? 1.0f : 0.0f), __float_as_uint(reached ? 1.0f : 0.0f),
                                    __float_as_uint(efirst), __float_as_uint(dist));
                dst[2] = make_uint4(__float_as_uint(emin), reason, __float_as_uint(st[(size_t)VF_TARGET_Y * n + e]),
                                    __float_as_uint(st[(size_t)VF_TARGET_Z * n + e]));
                dst[3] = make_uint4(__float_as_uint(st[(size_t)VF_OBJ_DEPTH * n + e]),
                                    __float_as_uint(st[(size_t)VF_OBJ_ANGLE * n + e]), 0u, 0u);
            }
        }

        // ---- the totals: this workgroup's finished episodes of this step, into row `chunk`
        if (b_done) {
            const double t_ret = wave_sum_f64(done ? (double)er : 0.0), t_len = wave_sum_f64(done ? (double)el : 0.0);
            const double t_first = wave_sum_f64(done ? (double)efirst : 0.0), t_fin = wave_sum_f64(done ? (double)dist : 0.0);
            const double t_min = wave_sum_f64(done ? (double)emin : 0.0);
            const unsigned long long b_ever = __ballot(done && efirst != 0.0f), b_end = __ballot(done && reached);
            const unsigned long long b_to = __ballot(to), b_lim = __ballot(limit_hit), b_tip = __ballot(tip_limit);
            const unsigned long long b_con = __ballot(contact);
            if (lane == 0) {
                double* r = red[wave];
                r[VINE_EVAL_EPISODES] = (double)__popcll(b_done);
                r[VINE_EVAL_RETURN_SUM] = t_ret;
                r[VINE_EVAL_LENGTH_SUM] = t_len;
                r[VINE_EVAL_REACHED_EVER] = (double)__popcll(b_ever);
                r[VINE_EVAL_REACHED_AT_END] = (double)__popcll(b_end);
                r[VINE_EVAL_FIRST_REACH_SUM] = t_first;
                r[VINE_EVAL_FINAL_DIST_SUM] = t_fin;
                r[VINE_EVAL_MIN_DIST_SUM] = t_min;
                r[VINE_EVAL_END_TIMEOUT] = (double)__popcll(b_to);
                r[VINE_EVAL_END_RAIL_LIMIT] = (double)__popcll(b_lim);
                r[VINE_EVAL_END_TIP_LIMIT] = (double)__popcll(b_tip);
                r[VINE_EVAL_END_CONTACT] = (double)__popcll(b_con);
            }
        } else if (lane < VINE_EVAL_NUM_TOTALS) {
            red[wave][lane] = 0.0;
        }
        __syncthreads();
        if (threadIdx.x < VINE_EVAL_NUM_TOTALS)
            totals[(size_t)chunk * VINE_EVAL_NUM_TOTALS + threadIdx.x] +=
                (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (SERIAL) __syncthreads();      // the next chunk writes wave_rows and red again
    }
    if (SERIAL && table && threadIdx.x == 0) cursor[0] = base0 + (unsigned long long)step_rows;
}

int validate(const VineEpisodesConfig* c) {
    if (!c) return vine_invalid_arg("episodes config is NULL");
    if (c->abi_version != VINE_EPISODES_ABI_VERSION) return vine_invalid_arg("VineEpisodesConfig.abi_version mismatch");
    if (c->reserved != 0) return vine_invalid_arg("VineEpisodesConfig.reserved must be 0");
    if (c->capacity < 1 || c->capacity > (int64_t)1 << 40) return vine_invalid_arg("episodes capacity out of range");
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_episodes_config_default(VineEpisodesConfig* c) {
    if (!c) return vine_invalid_arg("episodes config is NULL");
    c->abi_version = VINE_EPISODES_ABI_VERSION;
    c->reserved = 0;
    c->capacity = 1048576;
    return VINE_OK;
}

int vine_episodes_config_size(void) { return (int)sizeof(VineEpisodesConfig); }

int vine_episodes_rows(VineHandle* h) {
    if (!h) return vine_invalid_arg("null argument to vine_episodes_rows");
    VineHandleInfo info;
    const int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    return (info.n + THREADS - 1) / THREADS;
}

int64_t vine_episodes_table_bytes(const VineEpisodesConfig* c) {
    const int rc = validate(c);
    if (rc) return rc;
    return c->capacity * VINE_EPISODES_WORDS * (int64_t)sizeof(uint32_t);
}

int vine_episodes_scheduled(VineHandle* h, const VineEpisodesConfig* cfg, const float* rew, const int64_t* reset,
                            const int64_t* progress, const uint8_t* timeouts, float* episode, double* totals,
                            uint32_t* table, int64_t* cursor, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!h || !rew || !reset || !progress || !timeouts || !episode || !totals)
        return vine_invalid_arg("null argument to vine_episodes_scheduled");
    if ((table == nullptr) != (cursor == nullptr)) return vine_invalid_arg("episodes table and cursor go together: both or neither");
    if (reinterpret_cast<uintptr_t>(table) & 15u) return vine_invalid_arg("episodes table must be 16-byte aligned");
    VineHandleInfo info;
    rc = vine_handle_info(h, &info);
    if (rc) return rc;
    const float* rmat = vine_reward_matrix_of(h);
    if (!rmat)
        return vine_invalid_arg("vine_episodes_scheduled needs a reward matrix bound to the handle (vine_bind_reward_matrix) "
                                "before the step it accounts for");
    EpisodesParams E;
    E.n = info.n; E.glog = info.glog; E.nchunks = (info.n + THREADS - 1) / THREADS;
    E.flags = info.flags; E.capacity = cfg->capacity;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (table && cfg->capacity < info.n)      // one step could lap itself: one workgroup hands out the slots in env order
        hipLaunchKernelGGL(vine_episodes_kernel<true>, dim3(1), dim3(THREADS), 0, s, E, info.state, info.counters, rmat, rew,
                           (const long long*)reset, timeouts, episode, totals, (unsigned*)table, (unsigned long long*)cursor);
    else
        hipLaunchKernelGGL(vine_episodes_kernel<false>, dim3(E.nchunks), dim3(THREADS), 0, s, E, info.state, info.counters, rmat,
                           rew, (const long long*)reset, timeouts, episode, totals, (unsigned*)table,
                           (unsigned long long*)cursor);
    return vine_launch_status("vine_episodes");
}

}  // extern "C"
