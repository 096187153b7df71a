// env_draw_adr_host_check.cpp — the host-side entry points of csrc/vine_env_draw_adr.hip on their refusal paths, as a
// stand-alone program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/env_draw_adr_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_env_draw_adr.hip -o build/env_draw_adr_host_check
//   ./build/env_draw_adr_host_check
//
// The functions vine_env_draw_adr.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, as
// scripts/mpc_track_host_check.cpp does: a stand-in handle is a VineHandleInfo of this program's own making, and no reward
// matrix is ever bound to it.  The three observers' specs are made by hand (their units are not linked):
// vine_env_draw_adr_spec reads their abi_version, checked, seed, per_episode and names only.  Exit status 0 and
// "env draw adr host check ok" when every refusal is what include/vine_env_draw_adr.h says and a good spec comes out as the
// header states it.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/vine_env_draw_adr.h"
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
const float* vine_reward_matrix_of(VineHandle*) { return nullptr; }
int vine_env_tables_of(VineHandle*, const float** params, const float** inertia, unsigned* env_id_offset) {
    *params = *inertia = nullptr;
    *env_id_offset = 0u;
    return VINE_OK;
}
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_err);
    }
}

static VineEnvRedrawName range(double lo, double hi) {
    VineEnvRedrawName nm;
    memset(&nm, 0, sizeof nm);
    nm.form = VINE_REDRAW_RANGE;
    nm.key = 0x1234u;
    nm.radix = 1;
    nm.lo = lo;
    nm.hi = hi;
    return nm;
}

static VineConfig config() {
    VineConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_ABI_VERSION;
    c.seed = 7u;
    return c;
}

static VineEnvSensorSpec sensor_spec() {
    VineEnvSensorSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_SENSOR_ABI_VERSION;
    S.seed = 7u;
    S.per_episode = 1;
    S.checked = 1u;
    S.name[VSN_DELAY] = range(0.0, 3.0);
    S.name[VSN_HOLD] = range(0.0, 0.2);
    S.name[VSN_NOISE_STD] = range(0.0, 0.01);
    return S;
}

static VineEnvPushSpec push_spec() {
    VineEnvPushSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_PUSH_ABI_VERSION;
    S.seed = 7u;
    S.per_episode = 1;
    S.checked = 1u;
    S.name[VPU_RATE] = range(0.1, 0.1);
    S.name[VPU_RATE].form = VINE_REDRAW_NUMBER;
    S.name[VPU_IMPULSE] = range(0.0, 0.01);
    return S;
}

static VineEnvTargetSpec target_spec() {
    VineEnvTargetSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_TARGET_ABI_VERSION;
    S.seed = 7u;
    S.per_episode = 1;
    S.checked = 1u;
    S.name[VTG_VEL_ALONG] = range(-0.3, 0.3);
    S.name[VTG_VEL_ACROSS] = range(0.0, 0.0);
    S.name[VTG_SPAN_ALONG] = range(0.03, 0.04);
    S.name[VTG_SPAN_ACROSS] = range(0.0, 0.0);
    return S;
}

struct Names {
    VineEnvAdrName n[VDA_NAMES];
    Names() { memset(n, 0, sizeof n); }
    Names& on(int s, double lo, double hi, double step) {
        n[s].on = 1;
        n[s].start_lo = lo;
        n[s].start_hi = hi;
        n[s].step = step;
        return *this;
    }
};

static Names good() { return Names().on(VDA_SENSOR_DELAY, 1.0, 1.0, 1.0).on(VDA_PUSH_IMPULSE, 0.002, 0.004, 0.004).on(VDA_TARGET_VEL_ALONG, 0.0, 0.0, 0.05); }

static const VineConfig C0 = config();
static const VineEnvSensorSpec SE = sensor_spec();
static const VineEnvPushSpec PU = push_spec();
static const VineEnvTargetSpec TA = target_spec();

// the call with everything good but what the caller changes; refused with `word` in the text, and *out left unchecked
static bool refused(const VineConfig* c, const VineEnvSensorSpec* se, const VineEnvPushSpec* pu, const VineEnvTargetSpec* ta, const Names& names,
                    const char* word, double fraction = 0.25, int queue = 4, double widen_at = 0.8, double narrow_at = 0.4, int capacity = 64) {
    VineEnvDrawAdrSpec A;
    memset(&A, 0, sizeof A);
    g_err[0] = 0;
    return vine_env_draw_adr_spec(c, se, pu, ta, names.n, fraction, queue, widen_at, narrow_at, capacity, &A) == VINE_ERR_INVALID_ARG &&
           strstr(g_err, word) && A.checked == 0u;
}

alignas(16) static char buf[256];
static int32_t* const i32 = reinterpret_cast<int32_t*>(buf + 16);
static int64_t* const i64 = reinterpret_cast<int64_t*>(buf + 64);
static float* const f32 = reinterpret_cast<float*>(buf + 128);

int main() {
    expect(vine_env_draw_adr_spec_size() == (int)sizeof(VineEnvDrawAdrSpec) && sizeof(VineEnvDrawAdrSpec) == 1024 && sizeof(VineEnvDrawAdrSlot) == 104,
           "spec size");

    // a good spec
    VineEnvDrawAdrSpec A;
    memset(&A, 0xff, sizeof A);
    expect(vine_env_draw_adr_spec(&C0, &SE, &PU, &TA, good().n, 0.25, 4, 0.8, 0.4, 64, &A) == VINE_OK && A.checked == 1u, "a good spec");
    expect(A.abi_version == VINE_ENV_DRAW_ADR_ABI_VERSION && A.num_adr == 3 && A.queue == 4 && A.history_capacity == 64 && A.seed == 7u &&
               A.boundary_fraction == 0.25 && A.widen_at == 0.8 && A.narrow_at == 0.4,
           "the scalars of a good spec");
    expect(A.adr_slot[0] == VDA_SENSOR_DELAY && A.adr_slot[1] == VDA_PUSH_IMPULSE && A.adr_slot[2] == VDA_TARGET_VEL_ALONG && A.adr_slot[3] == -1 &&
               A.adr_slot[VDA_NAMES - 1] == -1,
           "adr_slot");
    expect(A.slot[VDA_SENSOR_DELAY].max_widen[0] == 1 && A.slot[VDA_SENSOR_DELAY].max_widen[1] == 2 && A.slot[VDA_SENSOR_DELAY].integer == 1 &&
               A.slot[VDA_PUSH_IMPULSE].max_widen[0] == 1 && A.slot[VDA_PUSH_IMPULSE].max_widen[1] == 2 &&
               A.slot[VDA_TARGET_VEL_ALONG].max_widen[0] == 6 && A.slot[VDA_TARGET_VEL_ALONG].max_widen[1] == 6,
           "max_widen");
    for (int s = 0; s < VDA_NAMES; ++s) {
        const int group = s < 3 ? VDA_SENSOR : s < 5 ? VDA_PUSH : VDA_TARGET, row = s < 3 ? s : s < 5 ? s - 3 : s - 5;
        expect(A.slot[s].group == group && A.slot[s].row == row && A.slot[s].integer == (s == 0) && A.slot[s].reserved == 0, "group, row and integer");
    }
    expect(A.slot[VDA_TARGET_VEL_ALONG].limits.lo == -0.3 && A.slot[VDA_TARGET_VEL_ALONG].limits.hi == 0.3 &&
               A.slot[VDA_TARGET_VEL_ALONG].limits.key == 0x1234u && A.slot[VDA_SENSOR_HOLD].adr.on == 0 && A.slot[VDA_SENSOR_HOLD].limits.hi == 0.2,
           "the limits are the observers' own names");
    // a group that is off and has no name under ADR
    expect(vine_env_draw_adr_spec(&C0, &SE, nullptr, nullptr, Names().on(VDA_SENSOR_NOISE_STD, 0.0, 0.0, 0.003).n, 0.0, 1, 0.8, 0.4, 1, &A) == VINE_OK &&
               A.num_adr == 1 && A.slot[VDA_SENSOR_NOISE_STD].max_widen[0] == 0 && A.slot[VDA_SENSOR_NOISE_STD].max_widen[1] == 4 &&
               A.slot[VDA_PUSH_IMPULSE].limits.form == VINE_REDRAW_ABSENT,
           "the sensor alone; the last step arrives at the limit");

    // refused by name
    expect(refused(nullptr, &SE, &PU, &TA, good(), "null argument to vine_env_draw_adr_spec"), "spec(NULL cfg)");
    g_err[0] = 0;
    expect(vine_env_draw_adr_spec(&C0, &SE, &PU, &TA, nullptr, 0.25, 4, 0.8, 0.4, 64, &A) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "spec(NULL names)");
    expect(vine_env_draw_adr_spec(&C0, &SE, &PU, &TA, good().n, 0.25, 4, 0.8, 0.4, 64, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "spec(NULL out)");
    {
        VineConfig c = C0;
        c.abi_version = 99;
        expect(refused(&c, &SE, &PU, &TA, good(), "VineConfig.abi_version mismatch"), "the config's abi");
        VineEnvSensorSpec se = SE;
        se.abi_version = 9;
        expect(refused(&C0, &se, &PU, &TA, good(), "VineEnvSensorSpec.abi_version mismatch"), "the sensor spec's abi");
        VineEnvPushSpec pu = PU;
        pu.abi_version = 9;
        expect(refused(&C0, &SE, &pu, &TA, good(), "VineEnvPushSpec.abi_version mismatch"), "the push spec's abi");
        VineEnvTargetSpec ta = TA;
        ta.abi_version = 9;
        expect(refused(&C0, &SE, &PU, &ta, good(), "VineEnvTargetSpec.abi_version mismatch"), "the target spec's abi");
        se = SE;
        se.checked = 0u;
        expect(refused(&C0, &se, &PU, &TA, good(), "was not filled by vine_env_sensor_spec"), "an unchecked sensor spec");
        pu = PU;
        pu.checked = 0u;
        expect(refused(&C0, &SE, &pu, &TA, good(), "was not filled by vine_env_push_spec"), "an unchecked push spec");
        ta = TA;
        ta.checked = 0u;
        expect(refused(&C0, &SE, &PU, &ta, good(), "was not filled by vine_env_target_spec"), "an unchecked target spec");
        ta = TA;
        ta.seed = 8u;
        expect(refused(&C0, &SE, &PU, &ta, good(), "seed is not the configuration's"), "another seed");
        expect(refused(&C0, nullptr, &PU, &TA, good(), "SENSOR_DELAY: a name under ADR needs its observer's spec"), "the sensor is off");
        expect(refused(&C0, &SE, nullptr, &TA, good(), "PUSH_IMPULSE: a name under ADR needs its observer's spec"), "the push is off");
        expect(refused(&C0, &SE, &PU, nullptr, good(), "TARGET_VEL_ALONG: a name under ADR needs its observer's spec"), "the target is off");
        ta = TA;
        ta.per_episode = 0;
        expect(refused(&C0, &SE, &PU, &ta, good(), "TARGET_VEL_ALONG: a name under ADR needs PER_EPISODE"), "held values");
        expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_RATE, 0.1, 0.1, 0.1), "PUSH_RATE: a name under ADR must be a [lo, hi] range"), "a number");
        se = SE;
        se.name[VSN_HOLD].form = VINE_REDRAW_VALUES;
        expect(refused(&C0, &se, &PU, &TA, Names().on(VDA_SENSOR_HOLD, 0.0, 0.1, 0.1), "SENSOR_HOLD: a name under ADR must be a [lo, hi] range"), "a value list");
    }
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, NAN, 0.004, 0.004), "PUSH_IMPULSE: START needs finite lo <= hi"), "START nan");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, 0.004, INFINITY, 0.004), "PUSH_IMPULSE: START needs finite lo <= hi"), "START inf");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, 0.004, 0.002, 0.004), "PUSH_IMPULSE: START needs finite lo <= hi"), "START lo > hi");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, -0.001, 0.002, 0.004), "PUSH_IMPULSE: START lies outside the limits"), "START below");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_TARGET_VEL_ALONG, 0.0, 0.31, 0.05), "TARGET_VEL_ALONG: START lies outside the limits"), "START above");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, 0.002, 0.004, 0.0), "PUSH_IMPULSE: STEP must be positive"), "STEP 0");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, 0.002, 0.004, -1.0), "PUSH_IMPULSE: STEP must be positive"), "STEP < 0");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, 0.002, 0.004, NAN), "PUSH_IMPULSE: STEP must be positive"), "STEP nan");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_PUSH_IMPULSE, 0.002, 0.004, INFINITY), "PUSH_IMPULSE: STEP must be positive"), "STEP inf");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_SENSOR_DELAY, 0.5, 1.0, 1.0), "SENSOR_DELAY: an integer parameter takes an integer START and STEP"), "START 0.5");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_SENSOR_DELAY, 1.0, 1.0, 0.5), "SENSOR_DELAY: an integer parameter takes an integer START and STEP"), "STEP 0.5");
    {
        Names off = good();
        off.n[VDA_SENSOR_HOLD].step = 0.1;
        expect(refused(&C0, &SE, &PU, &TA, off, "SENSOR_HOLD: START and STEP of a name that is not under ADR must be 0"), "STEP on a name that is off");
        off = good();
        off.n[VDA_TARGET_SPAN_ACROSS].start_hi = 1.0;
        expect(refused(&C0, &SE, &PU, &TA, off, "TARGET_SPAN_ACROSS: START and STEP of a name that is not under ADR must be 0"), "START on a name that is off");
        off = good();
        off.n[VDA_PUSH_RATE].reserved = 1;
        expect(refused(&C0, &SE, &PU, &TA, off, "PUSH_RATE: reserved must be 0"), "reserved");
    }
    expect(refused(&C0, &SE, &PU, &TA, Names(), "no name is under ADR"), "no name on");
    expect(refused(&C0, &SE, &PU, &TA, good(), "BOUNDARY_FRACTION must lie in [0, 1)", 1.0), "fraction 1");
    expect(refused(&C0, &SE, &PU, &TA, good(), "BOUNDARY_FRACTION must lie in [0, 1)", -0.1), "fraction < 0");
    expect(refused(&C0, &SE, &PU, &TA, good(), "BOUNDARY_FRACTION must lie in [0, 1)", NAN), "fraction nan");
    expect(refused(&C0, &SE, &PU, &TA, good(), "QUEUE must be at least 1", 0.25, 0), "queue 0");
    expect(refused(&C0, &SE, &PU, &TA, good(), "NARROW_AT must be below WIDEN_AT", 0.25, 4, 0.4, 0.4), "narrow = widen");
    expect(refused(&C0, &SE, &PU, &TA, good(), "NARROW_AT must be below WIDEN_AT", 0.25, 4, NAN, 0.4), "widen nan");
    expect(refused(&C0, &SE, &PU, &TA, good(), "NARROW_AT must be below WIDEN_AT", 0.25, 4, 0.8, -INFINITY), "narrow -inf");
    expect(refused(&C0, &SE, &PU, &TA, good(), "the history capacity must be at least 1", 0.25, 4, 0.8, 0.4, 0), "capacity 0");
    expect(refused(&C0, &SE, &PU, &TA, Names().on(VDA_TARGET_VEL_ALONG, 0.0, 0.0, 1e-11), "TARGET_VEL_ALONG: more than 2^30 STEPs"), "2^30 steps");

    // the launch's refusals, with a stand-in handle to which no reward matrix is bound
    expect(vine_env_draw_adr_spec(&C0, &SE, &PU, &TA, good().n, 0.25, 4, 0.8, 0.4, 64, &A) == VINE_OK, "a good spec for the launch");
    VineHandleInfo info;
    memset(&info, 0, sizeof info);
    info.n = 5;
    VineHandle* h = reinterpret_cast<VineHandle*>(&info);
    float* tables[VDA_GROUPS] = {f32, f32, f32};
#define NODE(handle, spec, reset, tabs, a0, a1, a2, a3, a4, a5, a6) \
    vine_env_draw_adr_scheduled(handle, spec, reset, tabs, nullptr, a0, a1, a2, a3, a4, a5, a6, nullptr)
#define NULLARG(call, what) expect((call) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_env_draw_adr_scheduled"), what)
    NULLARG(NODE(nullptr, &A, i64, tables, i32, i32, i32, i32, i32, i32, i64), "node(NULL handle)");
    NULLARG(NODE(h, nullptr, i64, tables, i32, i32, i32, i32, i32, i32, i64), "node(NULL spec)");
    NULLARG(NODE(h, &A, nullptr, tables, i32, i32, i32, i32, i32, i32, i64), "node(NULL reset)");
    NULLARG(NODE(h, &A, i64, nullptr, i32, i32, i32, i32, i32, i32, i64), "node(NULL tables)");
    NULLARG(NODE(h, &A, i64, tables, nullptr, i32, i32, i32, i32, i32, i64), "node(NULL widen)");
    NULLARG(NODE(h, &A, i64, tables, i32, nullptr, i32, i32, i32, i32, i64), "node(NULL counts)");
    NULLARG(NODE(h, &A, i64, tables, i32, i32, nullptr, i32, i32, i32, i64), "node(NULL reached)");
    NULLARG(NODE(h, &A, i64, tables, i32, i32, i32, nullptr, i32, i32, i64), "node(NULL probe)");
    NULLARG(NODE(h, &A, i64, tables, i32, i32, i32, i32, nullptr, i32, i64), "node(NULL episode_index)");
    NULLARG(NODE(h, &A, i64, tables, i32, i32, i32, i32, i32, nullptr, i64), "node(NULL history)");
    NULLARG(NODE(h, &A, i64, tables, i32, i32, i32, i32, i32, i32, nullptr), "node(NULL cursor)");
    for (int g = 0; g < VDA_GROUPS; ++g) {
        float* some[VDA_GROUPS] = {f32, f32, f32};
        some[g] = nullptr;
        NULLARG(NODE(h, &A, i64, some, i32, i32, i32, i32, i32, i32, i64), "node(NULL table of a group under ADR)");
        expect(strstr(g_err, g == 0 ? "SENSOR_DELAY is under ADR and needs the table of ENV_SENSOR"
                                    : g == 1 ? "PUSH_IMPULSE is under ADR and needs the table of ENV_PUSH"
                                             : "TARGET_VEL_ALONG is under ADR and needs the table of ENV_TARGET"),
               "the refusal names the name and the group");
    }
    VineEnvDrawAdrSpec bad = A;
    bad.checked = 0u;
    expect(NODE(h, &bad, i64, tables, i32, i32, i32, i32, i32, i32, i64) == VINE_ERR_INVALID_ARG && strstr(g_err, "was not filled by vine_env_draw_adr_spec"),
           "node: unchecked");
    bad = A;
    bad.abi_version = 7;
    expect(NODE(h, &bad, i64, tables, i32, i32, i32, i32, i32, i32, i64) == VINE_ERR_INVALID_ARG && strstr(g_err, "VineEnvDrawAdrSpec.abi_version mismatch"),
           "node: abi");
    for (int k = 0; k < 6; ++k) {
        bad = A;
        if (k == 0) bad.num_adr = 0;
        if (k == 1) bad.num_adr = 4;                       // (more than the slots that are on)
        if (k == 2) bad.adr_slot[1] = VDA_NAMES;
        if (k == 3) bad.slot[VDA_PUSH_IMPULSE].row = 5;
        if (k == 4) bad.slot[VDA_SENSOR_DELAY].limits.form = VINE_REDRAW_VALUES;
        if (k == 5) bad.history_capacity = 0;
        expect(NODE(h, &bad, i64, tables, i32, i32, i32, i32, i32, i32, i64) == VINE_ERR_INVALID_ARG &&
                   strstr(g_err, "lies outside what vine_env_draw_adr_spec fills"),
               "node: a spec altered behind the check");
    }
    // a group without a name under ADR needs no table
    {
        VineEnvDrawAdrSpec one;
        expect(vine_env_draw_adr_spec(&C0, &SE, nullptr, nullptr, Names().on(VDA_SENSOR_NOISE_STD, 0.0, 0.0, 0.003).n, 0.0, 1, 0.8, 0.4, 1, &one) == VINE_OK,
               "the sensor alone, for the launch");
        float* only[VDA_GROUPS] = {f32, nullptr, nullptr};
        expect(NODE(h, &one, i64, only, i32, i32, i32, i32, i32, i32, i64) == VINE_ERR_INVALID_ARG && strstr(g_err, "needs a reward matrix bound to the handle"),
               "node: no reward matrix (the last refusal in front of the launch)");
    }
    expect(NODE(h, &A, i64, tables, i32, i32, i32, i32, i32, i32, i64) == VINE_ERR_INVALID_ARG && strstr(g_err, "needs a reward matrix bound to the handle"),
           "node: no reward matrix");
    info.n = 0;
    expect(NODE(h, &A, i64, tables, i32, i32, i32, i32, i32, i32, i64) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "node: the handle's refusal passed on");

    if (failures) return 1;
    printf("env draw adr host check ok\n");
    return 0;
}
