// env_target_host_check.cpp — the host-side entry points of csrc/vine_env_target.hip on their refusal paths, as a stand-alone
// program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/env_target_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_env_target.hip -o build/env_target_host_check
//   ./build/env_target_host_check
//
// The functions vine_env_target.hip needs of vine_hip.hip (vine_observer.h, vine_inertia_composites.h, vine.h's vine_num_obs)
// are stood in for here, as scripts/mpc_filter_host_check.cpp does: a stand-in handle is a VineHandleInfo of this program's
// own making.  Exit status 0 and "env target host check ok" when every refusal is what include/vine_env_target.h says and a
// good spec comes out as the header states it.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/vine_env_target.h"
#include "../vine_robot_isaacgymenvs_amd/csrc/vine_observer.h"

static char g_err[256];
extern "C" {
void vine_set_error(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
int vine_handle_info(VineHandle* h, VineHandleInfo* out) {
    const VineHandleInfo* info = reinterpret_cast<const VineHandleInfo*>(h);
    if (info->n <= 0) {
        vine_set_error("stand-in handle");
        return VINE_ERR_INVALID_ARG;
    }
    *out = *info;
    return VINE_OK;
}
int vine_env_tables_of(VineHandle*, const float** params, const float** inertia, unsigned* env_id_offset) {
    *params = nullptr;
    *inertia = nullptr;
    *env_id_offset = 0;
    return VINE_OK;
}
int vine_num_obs(const VineConfig* cfg) {
    static const int columns[6] = {28, 18, 14, 26, 26, 26};
    return cfg->obs_type >= 0 && cfg->obs_type < 6 ? columns[cfg->obs_type] : -1;
}
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_err);
    }
}

static VineConfig config(unsigned flags, int obs_type = VINE_OBS_POS_AND_FD_VEL_AND_OBJ_INFO) {
    VineConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_ABI_VERSION;
    c.num_envs = 4;
    c.obs_type = obs_type;
    c.control_freq_inv = 4;
    c.dt = 0.00833f;
    c.clip_observations = 5.0f;
    c.flags = flags;
    c.seed = 11;
    for (int i = 0; i < VINE_MAX_OBS; ++i) c.obs_scaling[i] = 1.0f;
    c.obs_scaling[22] = 2.0f;
    c.obs_scaling[23] = 0.732f;
    return c;
}

struct Names {
    VineEnvRedrawName n[VTG_NAMES];
};
static VineEnvRedrawName number(double v) {
    VineEnvRedrawName nm;
    memset(&nm, 0, sizeof nm);
    nm.form = VINE_REDRAW_NUMBER;
    nm.lo = nm.hi = v;
    nm.radix = 1;
    return nm;
}
static VineEnvRedrawName range(double lo, double hi) {
    VineEnvRedrawName nm = number(lo);
    nm.form = VINE_REDRAW_RANGE;
    nm.hi = hi;
    return nm;
}
static VineEnvRedrawName list(int first, int count) {
    VineEnvRedrawName nm = number(0.0);
    nm.form = VINE_REDRAW_VALUES;
    nm.values_first = first;
    nm.values_count = count;
    return nm;
}
// VEL_ALONG 0.05 over a span of 0.03 m, nothing across
static Names good() {
    Names g;
    g.n[VTG_VEL_ALONG] = number(0.05);
    g.n[VTG_VEL_ACROSS] = number(0.0);
    g.n[VTG_SPAN_ALONG] = number(0.03);
    g.n[VTG_SPAN_ACROSS] = number(0.0);
    return g;
}

static const double kValues[4] = {0.0, 0.05, -0.05, 0.4};
static int spec_of(const VineConfig& c, const Names& g, int per_episode, VineEnvTargetSpec* out, int num_values = 4) {
    g_err[0] = 0;
    return vine_env_target_spec(&c, g.n, kValues, kValues, num_values, per_episode, out);
}
template <class Change>
static void refused(const char* word, Change change, unsigned flags = 0u, int per_episode = 0) {
    VineConfig c = config(flags);
    Names g = good();
    change(c, g);
    VineEnvTargetSpec S;
    expect(spec_of(c, g, per_episode, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, word), word);
}

alignas(16) static char buf[128];
static float* const p = reinterpret_cast<float*>(buf + 16);
static int64_t* const w = reinterpret_cast<int64_t*>(buf + 32);
static int32_t* const i32 = reinterpret_cast<int32_t*>(buf + 64);
static uint8_t* const u8 = reinterpret_cast<uint8_t*>(buf + 96);

int main() {
    typedef VineConfig C;
    typedef Names N;
    expect(vine_env_target_spec_size() == (int)sizeof(VineEnvTargetSpec), "spec size");

    // a good spec, in the three modes and the layouts
    VineEnvTargetSpec S;
    {
        VineConfig c = config(0u);
        expect(spec_of(c, good(), 0, &S) == VINE_OK && S.checked == 1u && S.mode == VINE_TARGET_FREE && S.vel_column == 22 && S.num_obs == 28,
               "free-space spec");
        expect(S.cdt == 0.00833f * 4.0f && S.inv_obs_scale[0] == (float)(1.0 / (double)2.0f) && S.inv_obs_scale[1] == (float)(1.0 / (double)0.732f),
               "cdt and the two reciprocals");
        c = config(VINE_FLAG_CREATE_SHELF, VINE_OBS_TIP_AND_CART_AND_OBJ_INFO);
        expect(spec_of(c, good(), 1, &S) == VINE_OK && S.mode == VINE_TARGET_SHELF && S.vel_column == 12 && S.per_episode == 1, "shelf spec");
        c = config(VINE_FLAG_CREATE_PIPE, VINE_OBS_POS_ONLY);
        expect(spec_of(c, good(), 0, &S) == VINE_OK && S.mode == VINE_TARGET_PIPE && S.vel_column == -1, "pipe spec, POS_ONLY");
        c = config(0u, VINE_OBS_POS_AND_PREV_POS);
        expect(spec_of(c, good(), 0, &S) == VINE_OK && S.vel_column == 22 && S.num_obs == 26, "26-column spec");
        // all velocities zero is a spec with per_episode; a value list with both signs and zero
        Names g = good();
        g.n[VTG_VEL_ALONG] = number(0.0);
        expect(spec_of(config(0u), g, 1, &S) == VINE_OK, "all zero, per episode");
        g.n[VTG_VEL_ALONG] = list(0, 3);
        expect(spec_of(config(0u), g, 0, &S) == VINE_OK, "value list");
        // a step that lands exactly on 2 * SPAN is not refused
        g = good();
        g.n[VTG_VEL_ALONG] = number(1.0);
        g.n[VTG_SPAN_ALONG] = number((double)(0.00833f * 4.0f) * 0.5);
        expect(spec_of(config(0u), g, 0, &S) == VINE_OK, "max|VEL| * cdt == 2 * SPAN");
    }

    // refused by name
    refused("TARGET_VEL_ALONG: absent", [](C&, N& g) { g.n[VTG_VEL_ALONG].form = VINE_REDRAW_ABSENT; });
    refused("TARGET_SPAN_ACROSS: unknown form", [](C&, N& g) { g.n[VTG_SPAN_ACROSS].form = 9; });
    refused("TARGET_VEL_ACROSS: reserved must be 0", [](C&, N& g) { g.n[VTG_VEL_ACROSS].reserved = 1; });
    refused("TARGET_VEL_ALONG: the number is not finite", [](C&, N& g) { g.n[VTG_VEL_ALONG] = number(NAN); });
    refused("TARGET_SPAN_ALONG: the number is not finite", [](C&, N& g) { g.n[VTG_SPAN_ALONG] = number(INFINITY); });
    refused("TARGET_VEL_ALONG: a range needs finite lo <= hi", [](C&, N& g) { g.n[VTG_VEL_ALONG] = range(0.05, -0.05); });
    refused("TARGET_SPAN_ALONG: a range needs finite lo <= hi", [](C&, N& g) { g.n[VTG_SPAN_ALONG] = range(0.03, INFINITY); });
    refused("TARGET_SPAN_ALONG: must not be negative", [](C&, N& g) { g.n[VTG_SPAN_ALONG] = number(-0.03); });
    refused("TARGET_SPAN_ACROSS: must not be negative", [](C&, N& g) { g.n[VTG_SPAN_ACROSS] = range(-0.01, 0.02); });
    refused("TARGET_SPAN_ALONG: must not be negative", [](C&, N& g) { g.n[VTG_SPAN_ALONG] = list(2, 2); });
    refused("TARGET_VEL_ALONG: the extent of the value list", [](C&, N& g) { g.n[VTG_VEL_ALONG] = list(2, 3); });
    refused("TARGET_VEL_ALONG: the extent of the value list", [](C&, N& g) { g.n[VTG_VEL_ALONG] = list(-1, 2); });
    refused("TARGET_VEL_ALONG: the extent of the value list", [](C&, N& g) { g.n[VTG_VEL_ALONG] = list(0, 0); });
    refused("TARGET_VEL_ALONG: radix must be at least 1", [](C&, N& g) { g.n[VTG_VEL_ALONG] = list(0, 3); g.n[VTG_VEL_ALONG].radix = 0; });
    refused("TARGET_VEL_ALONG: does not fit a float32", [](C&, N& g) { g.n[VTG_VEL_ALONG] = number(1e300); });
    // the path: a step longer than the path, a moving axis without a span, on either axis
    refused("TARGET_VEL_ALONG: max|VEL| * cdt exceeds 2 * min SPAN_ALONG", [](C&, N& g) { g.n[VTG_VEL_ALONG] = number(2.0); });
    refused("TARGET_VEL_ALONG: max|VEL| * cdt exceeds 2 * min SPAN_ALONG", [](C&, N& g) { g.n[VTG_VEL_ALONG] = list(1, 3); g.n[VTG_SPAN_ALONG] = number(0.006); });
    refused("TARGET_VEL_ALONG: max|VEL| * cdt exceeds 2 * min SPAN_ALONG", [](C&, N& g) { g.n[VTG_SPAN_ALONG] = range(0.0, 0.03); });
    refused("TARGET_VEL_ACROSS: max|VEL| * cdt exceeds 2 * min SPAN_ACROSS", [](C&, N& g) { g.n[VTG_VEL_ACROSS] = range(-0.01, 0.0); });
    // with an obstacle nothing moves across
    refused("TARGET_VEL_ACROSS: must be constant zero with an obstacle",
            [](C&, N& g) { g.n[VTG_VEL_ACROSS] = number(0.01); g.n[VTG_SPAN_ACROSS] = number(0.01); }, VINE_FLAG_CREATE_SHELF);
    refused("TARGET_SPAN_ACROSS: must be constant zero with an obstacle", [](C&, N& g) { g.n[VTG_SPAN_ACROSS] = number(0.01); }, VINE_FLAG_CREATE_PIPE);
    refused("CREATE_SHELF together with CREATE_PIPE", [](C&, N&) {}, VINE_FLAG_CREATE_SHELF | VINE_FLAG_CREATE_PIPE);
    // nothing to do; the step's velocity term
    refused("TARGET_VEL_ALONG and TARGET_VEL_ACROSS are both constant zero: nothing to do", [](C&, N& g) { g.n[VTG_VEL_ALONG] = number(0.0); });
    refused("TARGET_VEL_ALONG and TARGET_VEL_ACROSS are both constant zero: nothing to do", [](C&, N& g) { g.n[VTG_VEL_ALONG] = list(0, 1); });
    refused("VELOCITY_SUCCESS_REWARD_WEIGHT must be 0", [](C& c, N&) { c.reward_weights[3] = 0.5f; }, 0u, 1);
    refused("clip_observations must be positive", [](C& c, N&) { c.clip_observations = 0.0f; });
    refused("dt * controlFrequencyInv must be positive", [](C& c, N&) { c.control_freq_inv = 0; });
    refused("no known layout", [](C& c, N&) { c.obs_type = 6; });
    {
        VineConfig c = config(0u);
        Names g = good();
        expect(vine_env_target_spec(nullptr, g.n, kValues, kValues, 4, 0, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "spec(NULL cfg)");
        expect(vine_env_target_spec(&c, g.n, nullptr, kValues, 4, 0, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "a host and a device array"),
               "spec(NULL host values)");
        expect(vine_env_target_spec(&c, g.n, kValues, kValues, -1, 0, &S) == VINE_ERR_INVALID_ARG, "spec(negative num_values)");
    }

    // the launch's refusals, with a stand-in handle
    VineConfig c = config(VINE_FLAG_CREATE_PIPE);
    expect(spec_of(c, good(), 0, &S) == VINE_OK, "a pipe spec for the launch");
    VineHandleInfo info;
    memset(&info, 0, sizeof info);
    info.n = 4;
    info.flags = VINE_FLAG_CREATE_PIPE;
    VineHandle* h = reinterpret_cast<VineHandle*>(&info);
    expect(vine_env_target_scheduled(h, &S, nullptr, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "null argument to vine_env_target_scheduled"), "scheduled(NULL obs)");
    expect(vine_env_target_scheduled(nullptr, &S, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"),
           "scheduled(NULL handle)");
    VineEnvTargetSpec bad = S;
    bad.abi_version = 7;
    expect(vine_env_target_scheduled(h, &bad, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "abi_version mismatch"), "abi");
    bad = S;
    bad.checked = 0u;
    expect(vine_env_target_scheduled(h, &bad, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "was not filled by vine_env_target_spec"), "unchecked spec");
    bad = S;
    bad.num_values = 2;
    bad.values = nullptr;
    expect(vine_env_target_scheduled(h, &bad, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "values is NULL"), "values");
    bad = S;
    bad.vel_column = 27;
    expect(vine_env_target_scheduled(h, &bad, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "vel_column lies outside the observation row"), "vel_column");
    info.flags = VINE_FLAG_CREATE_SHELF;
    expect(vine_env_target_scheduled(h, &S, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "mode is not that of the handle's obstacle flags"), "mode against the handle");
    info.flags = VINE_FLAG_CREATE_PIPE;
    info.n = 0;
    expect(vine_env_target_scheduled(h, &S, p, w, w, p, p, u8, i32, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "the handle's refusal passed on");

    if (failures) return 1;
    printf("env target host check ok\n");
    return 0;
}
