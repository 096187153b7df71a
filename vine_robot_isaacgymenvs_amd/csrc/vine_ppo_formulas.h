// vine_ppo_formulas.h — the pointwise formulas of the update and inference kernels (ppo_kernels.hip), each stated once.
// The kernels keep their own layouts, loads, reductions and stores; what tests compare bit for bit between two routes
// (the LSTM sequence kernels against the step kernels, the fused LayerNorm + heads + loss against the stand-alone kernels,
// the one-launch MLPs against normalize_obs_kernel) is the arithmetic below.  Inlined device functions only; operands by
// reference (by value the compiler picked another contraction: profiles/step_task_once/checks.txt), no __restrict__.
#ifndef VINE_PPO_FORMULAS_H
#define VINE_PPO_FORMULAS_H

#include <hip/hip_runtime.h>

// v_rcp_f32 (1 ulp) instead of the IEEE division sequence (~10 VALU instructions): the LSTM step kernel spent 800 of
// its 1800 VALU instructions per wave on the 80 divisions of its gate non-linearities
__device__ __forceinline__ float rcpf_(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sigmoidf_(float x) { return rcpf_(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) {
    // tanh via exp of -2|x|: accurate to ~2e-7 relative, no overflow
    const float ax = fabsf(x);
    const float e = __expf(-2.0f * ax);
    const float t = (1.0f - e) * rcpf_(1.0f + e);
    return copysignf(t, x);
}

// ---- LSTM cell.  Forward, from the four pre-activations (bias added by the caller) and the cell state the step keeps
// (c_kept = keep * c_{t-1}, formed by the caller): the gate activations, c_t and h_t.
// An output may be the object of an input (lstm_fwd_kernel writes each activation over its pre-activation), and that is
// part of a caller's bits: under -ffp-contract=fast c_t is one product rounded and one fma, and WHICH product is rounded
// follows the call site.  In place it is gi gg, as in the step kernels; with fresh arrays lstm_fwd_kernel rounded
// gf c_kept instead -- the same opcodes, other bits.  Keep a caller's form when touching it.
__device__ __forceinline__ void lstm_cell(const float& pi, const float& pf, const float& pg, const float& po,
                                          const float& c_kept, float& gi, float& gf, float& gg, float& go, float& c_new,
                                          float& h_new) {
    gi = sigmoidf_(pi);
    gf = sigmoidf_(pf);
    gg = tanhf_(pg);
    go = sigmoidf_(po);
    c_new = gf * c_kept + gi * gg;
    h_new = go * tanhf_(c_new);
}
// Backward, from dh = d loss / d h_t (recurrent part added by the caller), dc = the masked d loss / d c_t carried from step
// t + 1, the saved gate activations, c_t and c_kept: the gradients of the four pre-activations and d loss / d c_kept.
__device__ __forceinline__ void lstm_cell_bwd(const float& dh, const float& dc, const float& c_new, const float& c_kept,
                                              const float& gi, const float& gf, const float& gg, const float& go, float& di,
                                              float& df, float& dg, float& dout, float& dc_kept) {
    const float tc = tanhf_(c_new);
    const float d_o = dh * tc;
    const float d_c = dc + dh * go * (1.0f - tc * tc);
    di = d_c * gg * gi * (1.0f - gi);
    df = d_c * c_kept * gf * (1.0f - gf);
    dg = d_c * gi * (1.0f - gg * gg);
    dout = d_o * go * (1.0f - go);
    dc_kept = d_c * gf;
}

// ---- ELU, and its derivative from the OUTPUT a = elu(z)
__device__ __forceinline__ float elu1(float x, float alpha) { return x > 0.0f ? x : alpha * (__expf(x) - 1.0f); }
__device__ __forceinline__ float elu_grad(float a, float alpha) { return a > 0.0f ? 1.0f : a + alpha; }

// ---- observation normaliser (RunningMeanStd in eval mode, rl_games: float64 statistics cast to float FIRST, then
// clamp((x - mean) / sqrt(var + eps), +-clip))
__device__ __forceinline__ float obs_std(double var, float eps) { return sqrtf((float)var + eps); }
__device__ __forceinline__ float obs_normalize(const float& x, const float& mean, const float& sd, float clip) {
    return fminf(fmaxf((x - mean) / sd, -clip), clip);
}

// ---- LayerNorm of a row of H values, two-pass: the caller sums (wave_sum and row_allsum16 add in different orders),
// centres with mean = sum / H and hands the sum of the squared centred values to layernorm_rstd
__device__ __forceinline__ float layernorm_rstd(float sum_sq, int H, float eps) { return rsqrtf(sum_sq * (1.0f / H) + eps); }
__device__ __forceinline__ float layernorm_affine(const float& x_centred, const float& rstd, const float& gamma, const float& beta) {
    return x_centred * rstd * gamma + beta;
}

// ---- PPO loss.  A workgroup of a loss kernel leaves one row of PPO_LOSS_ROW partial sums, folded by ppo_loss_finalize:
//   slot 0..3 actor, critic, bound loss and KL (sums over the samples), 4 unused,
//   PPO_SLOT_GLS + k      d loss / d logstd[k]       (k < A <= PPO_MAX_A; the slots of k >= A hold zeros)
//   PPO_SLOT_GMU + k      column sum of d loss / d mu[:, k] (the mu head's bias gradient)
//   PPO_SLOT_GV           sum of d loss / d value     (the value head's bias gradient)
#define PPO_MAX_A 8
#define PPO_LOSS_ROW 32          // floats per row (PPO_NRED used)
constexpr int PPO_SLOT_GLS = 5, PPO_SLOT_GMU = 5 + PPO_MAX_A, PPO_SLOT_GV = 5 + 2 * PPO_MAX_A, PPO_NRED = PPO_SLOT_GV + 1;
// slots that can be non-zero with A actions: the others skip their reductions (A is uniform, so is the branch)
__device__ __forceinline__ bool ppo_slot_live(int q, int A) {
    return q < 4 || (q >= PPO_SLOT_GLS && q < PPO_SLOT_GLS + A) || (q >= PPO_SLOT_GMU && q < PPO_SLOT_GMU + A) ||
           q == PPO_SLOT_GV;
}
__device__ __forceinline__ void ppo_sigma(const float& logstd, float& sg, float& isg2) {
    sg = __expf(logstd);
    isg2 = 1.0f / (sg * sg);
}
// One sample, in the pieces that a loss kernel calls from its own loops over the A actions (the kernels keep their loops,
// their loads and the order of their stores): ppo_z2 per action, then the two scalar pieces, then ppo_g_mu, ppo_g_logstd
// and ppo_kl per action.  Gradients carry 1 / n, not the loss scale.  nlp starts from the caller's constant part of
// -log p, 0.5 log(2 pi) A + sum logstd -- each kernel adds that up in its own order and keeps its bits.
__device__ __forceinline__ void ppo_z2(const float& act, const float& mu, const float& isg2, float& dm, float& z2, float& nlp) {
    dm = act - mu;
    z2 = dm * dm * isg2;
    nlp += 0.5f * z2;
}
// ratio and clipped surrogate: the actor loss and d loss / d nlp
__device__ __forceinline__ void ppo_surrogate(const float& nlp, const float& old_neglogp, const float& adv, float e_clip,
                                              float inv_n, float& a_loss, float& dL_dnlp) {
    const float a = adv;
    const float ratio = __expf(old_neglogp - nlp);
    const float rc = fminf(fmaxf(ratio, 1.0f - e_clip), 1.0f + e_clip);
    const float s1 = -a * ratio, s2 = -a * rc;
    const bool first = s1 >= s2;                     // torch.max sends the tie's gradient to the first operand
    a_loss = first ? s1 : s2;
    const float inside = (ratio > 1.0f - e_clip && ratio < 1.0f + e_clip) ? 1.0f : 0.0f;
    const float dL_dratio = first ? -a : -a * inside;
    dL_dnlp = -ratio * dL_dratio * inv_n;            // d ratio / d nlp = -ratio
}
// clipped or plain value loss and d loss / d value
__device__ __forceinline__ void ppo_value_loss(const float& value, const float& old_value, const float& ret, float e_clip,
                                               int clip_value, float critic_coef, float inv_n, float& c_loss, float& g_value) {
    const float v = value, vp = old_value, R = ret;
    float dL_dv;
    if (clip_value) {
        const float dv = v - vp;
        const float vc = vp + fminf(fmaxf(dv, -e_clip), e_clip);
        const float l1 = (v - R) * (v - R), l2 = (vc - R) * (vc - R);
        if (l1 >= l2) { c_loss = l1; dL_dv = 2.0f * (v - R); }
        else { c_loss = l2; dL_dv = (dv > -e_clip && dv < e_clip) ? 2.0f * (vc - R) : 0.0f; }
    } else {
        c_loss = (R - v) * (R - v);
        dL_dv = 2.0f * (v - R);
    }
    g_value = 0.5f * critic_coef * dL_dv * inv_n;
}
// bound loss of one action, added to b_loss, and d loss / d mu[k]  (d nlp / d mu = -(a - mu) / sigma^2)
__device__ __forceinline__ float ppo_g_mu(const float& m, const float& dm, const float& isg2, const float& dL_dnlp,
                                          float bounds_coef, float soft_bound, float inv_n, float& b_loss) {
    const float hi = fmaxf(m - soft_bound, 0.0f), lo = fminf(m + soft_bound, 0.0f);
    b_loss += hi * hi + lo * lo;
    return dL_dnlp * (-dm * isg2) + bounds_coef * inv_n * 2.0f * (hi + lo);
}
__device__ __forceinline__ float ppo_g_logstd(const float& dL_dnlp, const float& z2) { return dL_dnlp * (1.0f - z2); }      // d nlp / d logstd = 1 - z^2
// KL of one action against the old (mu, sigma), added to kl
__device__ __forceinline__ void ppo_kl(const float& m, const float& sg, const float& om, const float& os, float& kl) {
    const float c1 = __logf(os / sg + 1e-5f);
    const float c2 = (sg * sg + (om - m) * (om - m)) / (2.0f * (os * os + 1e-5f));
    kl += c1 + c2 - 0.5f;
}

#endif
