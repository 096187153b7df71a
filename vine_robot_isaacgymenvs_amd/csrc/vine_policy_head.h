// vine_policy_head.h — the rollout's policy head, its action sampling and its step bookkeeping, each stated once: for
// policy_head_kernel, policy_head16_kernel and rollout_post_kernel (ppo_kernels.hip) and for the ROLL and EVAL blocks of
// vine_step_quad_kernel (vine_hip.hip).  The kernels differ in how they lay a row over lanes and in how they reduce; the
// formulas that tests compare bit for bit between them are here.  Inlined device functions only; accumulated or indexed
// operands by reference (by value the compiler picked another contraction: profiles/step_task_once/checks.txt).
#ifndef VINE_POLICY_HEAD_H
#define VINE_POLICY_HEAD_H

#include <hip/hip_runtime.h>

// ---- random numbers
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }
// The two action-noise streams, keyed by (seed_lo, seed_hi); the counter words of a draw (the step kernels' own streams are
// rng4() in vine_hip.hip):
//   rollout:     (env, counter, RNG_POLICY_ACTION, k >> 1)      the rollout's step count; one draw serves components k, k + 1
//   evaluation:  (env, step,    RNG_EVAL_ACTION,   step >> 32)  the handle's own 64-bit step count
#define RNG_POLICY_ACTION 0x504f4c59u      // "POLY"
#define RNG_EVAL_ACTION 0x4556414cu        // "EVAL"
__device__ __forceinline__ void rng_policy_action(unsigned env, unsigned long long counter, unsigned pair, unsigned seed_lo,
                                                  unsigned seed_hi, unsigned out[4]) {
    philox4x32_10(env, (unsigned)counter, RNG_POLICY_ACTION, pair, seed_lo, seed_hi, out);
}
__device__ __forceinline__ void rng_eval_action(unsigned env, unsigned long long step, unsigned seed_lo, unsigned seed_hi,
                                                unsigned out[4]) {
    philox4x32_10(env, (unsigned)step, RNG_EVAL_ACTION, (unsigned)(step >> 32), seed_lo, seed_hi, out);
}
// Two standard normal deviates from two random words (Box-Muller on the hardware's log / sin / cos; u1 in (0, 1]).
__device__ __forceinline__ void action_noise_pair(unsigned r0, unsigned r1, float& e0, float& e1) {
    const float u1 = 1.0f - u01(r0), u2 = u01(r1);
    const float rad = sqrtf(-2.0f * __logf(u1));
    float sn, cs;
    __sincosf(6.283185307179586f * u2, &sn, &cs);
    e0 = rad * cs; e1 = rad * sn;
}
// ---- value and likelihood
// RunningMeanStd(value) inverted, from its own float64 statistics (mean.float(), sqrt(var.float() + eps)) ...
__device__ __forceinline__ float unnormalize_value(float v, const double* mean, const double* var, float eps) {
    const float vm = (float)mean[0], vs = sqrtf((float)var[0] + eps);
    return fminf(fmaxf(v, -5.0f), 5.0f) * vs + vm;
}
// ... or from a float mean and standard deviation
__device__ __forceinline__ float unnormalize_value(float v, float mean, float std) {
    return fminf(fmaxf(v, -5.0f), 5.0f) * std + mean;
}
// -log N(a; mu, sigma) summed over A components = gauss_neglogp_const(A) + sum_k gauss_neglogp(noise_k, log sigma_k),
// with noise = (a - mu) / sigma
__device__ __forceinline__ float gauss_neglogp_const(int A) { return 0.9189385332046727f * A; }      // 0.5 log(2 pi) A
__device__ __forceinline__ float gauss_neglogp(float noise, float logstd) { return 0.5f * noise * noise + logstd; }
// The lane that holds env e's reduced head rows (acc[k] = w_mu[k] . y for k < A, acc[MAXA] = w_v . y) finishes the head:
// value (normalize_value: 0 as it is, 2 float64 statistics, else two floats), then one draw per pair of components.
template <int MAXA>
__device__ __forceinline__ void head_tail(long long e, int A, const float (&acc)[MAXA + 1], const float* b_mu, const float* b_v,
                                          const float* logstd, const float* vmean, const float* vstd, int normalize_value,
                                          float value_eps, unsigned seed_lo, unsigned seed_hi, unsigned long long ctr,
                                          float* mu_out, float* sigma_out, float* value_out, float* action_out,
                                          float* neglogp_out) {
    float v = acc[MAXA] + b_v[0];
    if (normalize_value == 2)
        v = unnormalize_value(v, reinterpret_cast<const double*>(vmean), reinterpret_cast<const double*>(vstd), value_eps);
    else if (normalize_value) v = unnormalize_value(v, vmean[0], vstd[0]);
    value_out[e] = v;
    float nlp = gauss_neglogp_const(A);
    unsigned r[4];
    for (int k = 0; k < A; k += 2) {
        rng_policy_action((unsigned)e, ctr, (unsigned)(k >> 1), seed_lo, seed_hi, r);
        float eps2[2];
        action_noise_pair(r[0], r[1], eps2[0], eps2[1]);
        for (int q = 0; q < 2 && k + q < A; ++q) {
            const int kk = k + q;
            const float m = acc[kk] + b_mu[kk], ls = logstd[kk], sg = __expf(ls);
            const float a = m + sg * eps2[q];
            mu_out[e * A + kk] = m;
            sigma_out[e * A + kk] = sg;
            action_out[e * A + kk] = a;
            nlp += gauss_neglogp(eps2[q], ls);
        }
    }
    neglogp_out[e] = nlp;
}
// ---- four lanes per env (vine_step_quad_kernel).  Cross-lane operands are DPP quad_perm sources: a DPP read needs the whole
// quad active (a lane that EXEC has switched off delivers 0), so what reduces over the quad is called from quad-uniform
// control flow (NOTE on selects, vine_hip.hip).
template <int CTRL>
__device__ __forceinline__ float qperm(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_sum(float v) {
    const float s = v + qperm<0xB1>(v);                                                    // xor 1
    return s + qperm<0x4E>(s);                                                             // xor 2
}
// LayerNorm + heads of one 256-unit row held by a quad: lane t holds units {16 i + 4 t .. + 3 : i < 16} in yq[i].  Two
// passes (mean, then the centred second moment and NROWS centred dot products with hw[k][u] = gamma_u w_k[u]);
// out[k] = rstd * (hw[k] . (y - mean)) + hc[k] with hc[k] = w_k . beta + b_k (vine_rollout_head_prep).
template <int NROWS>
__device__ __forceinline__ void quad_ln_heads(const float4 (&yq)[16], const float* hw, int t, float ln_eps,
                                              const float* hc, float (&out)[NROWS]) {
    float s1 = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s1 += (yq[i].x + yq[i].y) + (yq[i].z + yq[i].w);
    const float mean = quad_sum(s1) * (1.0f / 256.0f);
    float q2 = 0.0f, d[NROWS] = {};
    const float4* hw0 = reinterpret_cast<const float4*>(hw) + t;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float4 w[NROWS];
#pragma unroll
        for (int k = 0; k < NROWS; ++k) w[k] = hw0[64 * k + 4 * i];
        const float c0 = yq[i].x - mean, c1 = yq[i].y - mean, c2 = yq[i].z - mean, c3 = yq[i].w - mean;
        q2 += (c0 * c0 + c1 * c1) + (c2 * c2 + c3 * c3);
#pragma unroll
        for (int k = 0; k < NROWS; ++k) d[k] += (c0 * w[k].x + c1 * w[k].y) + (c2 * w[k].z + c3 * w[k].w);
    }
    const float rstd = rsqrtf(quad_sum(q2) * (1.0f / 256.0f) + ln_eps);
#pragma unroll
    for (int k = 0; k < NROWS; ++k) out[k] = rstd * quad_sum(d[k]) + hc[k];
}
// The LSTM-state rows of a finished env (H == 256, fp32) cleared by its four lanes, and the operand copy of h that the
// next inference step reads, if there is one.  (rollout_post_kernel clears with 16 lanes per env, any H, fp32 or bf16.)
__device__ __forceinline__ void quad_clear_lstm_rows(float* h_state, float* c_state,
                                                     float* h_op, long long h_op_stride, int e, int t) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4* hr = reinterpret_cast<float4*>(h_state + (size_t)e * 256) + t;
    float4* cr4 = reinterpret_cast<float4*>(c_state + (size_t)e * 256) + t;
#pragma unroll
    for (int i = 0; i < 16; ++i) { hr[4 * i] = z; cr4[4 * i] = z; }
    if (h_op) {
        float4* orow = reinterpret_cast<float4*>(h_op + (size_t)e * h_op_stride) + t;
#pragma unroll
        for (int i = 0; i < 16; ++i) orow[4 * i] = z;
    }
}
// ---- step bookkeeping (play_steps_rnn; rl_games common_agent.py:293-306), one env, one step.  Returns the shaped reward with
// the time-out bootstrap gamma_b * value; *timeout and *value are pointers because they are read only where needed (a
// reference would license the compiler to load through a NULL `values`).  cur_r / cur_l: the running episode's return and
// length, in and out; fin_r / fin_l: the episode's totals with this step, which count when `done`.
__device__ __forceinline__ float rollout_book(float r, bool done, const unsigned char* timeout, const float* value, float shift,
                                              float scale, float gamma_b, float& cur_r, float& cur_l, float& fin_r,
                                              float& fin_l) {
    float s = (r + shift) * scale;
    if (gamma_b != 0.0f && *timeout) s += gamma_b * *value;
    fin_r = cur_r + r; fin_l = cur_l + 1.0f;
    cur_r = done ? 0.0f : fin_r; cur_l = done ? 0.0f : fin_l;
    return s;
}
// A 256-thread workgroup's row of `partial`, {sum of finished returns, sum of finished lengths, count}, from each wave's v3:
// the wave reduction stays the kernel's own (its summation order shows in the meters, which tests compare bit for bit).
__device__ __forceinline__ void store_block_row3(float (&red)[4][3], const float (&v3)[3], float* row) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = v3[0]; red[wave][1] = v3[1]; red[wave][2] = v3[2]; }
    __syncthreads();
    if (threadIdx.x < 3)
        row[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
#endif
