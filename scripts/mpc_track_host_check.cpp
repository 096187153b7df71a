// mpc_track_host_check.cpp — the host-side entry points of csrc/vine_mpc_track.hip on their refusal paths, as a stand-alone
// program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_track_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc_track.hip -o build/mpc_track_host_check
//   ./build/mpc_track_host_check
//
// The functions vine_mpc_track.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, as
// scripts/env_target_host_check.cpp does: a stand-in handle is a VineHandleInfo of this program's own making.  The plant's
// target spec is made by hand too (vine_env_target.hip is not linked): vine_mpc_track_spec reads its abi_version, checked, mode
// and cdt only.  Exit status 0 and "mpc track host check ok" when every refusal is what include/vine_mpc_track.h says and a
// good spec comes out as the header states it.
#include <cstdio>
#include <cstring>

#include "../include/vine_mpc_track.h"
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
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_err);
    }
}

static VineEnvTargetSpec plant_spec(int mode) {
    VineEnvTargetSpec T;
    memset(&T, 0, sizeof T);
    T.abi_version = VINE_ENV_TARGET_ABI_VERSION;
    T.mode = mode;
    T.cdt = 0.00833f * 4.0f;
    T.checked = 1u;
    return T;
}

static VineMpcConfig config(int m, int k, int h) {
    VineMpcConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_MPC_ABI_VERSION;
    c.num_plants = m;
    c.samples = k;
    c.horizon = h;
    c.lambda = 0.05;
    c.sigma[0] = c.sigma[1] = 0.5f;
    return c;
}

static bool refused_spec(const VineEnvTargetSpec* T, const VineMpcConfig* c, int path, const char* word) {
    VineMpcTrackSpec S;
    memset(&S, 0, sizeof S);
    g_err[0] = 0;
    return vine_mpc_track_spec(T, c, path, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, word) && S.checked == 0u;
}

alignas(16) static char buf[128];
static float* const p = reinterpret_cast<float*>(buf + 16);
static int64_t* const w = reinterpret_cast<int64_t*>(buf + 32);
static uint8_t* const u8 = reinterpret_cast<uint8_t*>(buf + 96);

int main() {
    expect(vine_mpc_track_spec_size() == (int)sizeof(VineMpcTrackSpec) && sizeof(VineMpcTrackSpec) == 64, "spec size");

    // a good spec, in the three modes and the three kinds
    VineMpcTrackSpec S;
    for (int mode = VINE_TARGET_FREE; mode <= VINE_TARGET_PIPE; ++mode)
        for (int path = VINE_TRACK_EXACT; path <= VINE_TRACK_HELD; ++path) {
            const VineEnvTargetSpec T = plant_spec(mode);
            const VineMpcConfig c = config(5, 14, 12);
            memset(&S, 0xff, sizeof S);
            expect(vine_mpc_track_spec(&T, &c, path, &S) == VINE_OK && S.checked == 1u && S.abi_version == VINE_MPC_TRACK_ABI_VERSION &&
                       S.num_plants == 5 && S.samples == 14 && S.horizon == 12 && S.mode == mode && S.path == path && S.cdt == T.cdt,
                   "a good spec");
            for (int i = 0; i < 8; ++i) expect(S.reserved[i] == 0u, "reserved words are zero");
        }
    {
        const VineEnvTargetSpec T = plant_spec(VINE_TARGET_FREE);
        VineMpcConfig c = config(1, 2, 1);
        expect(vine_mpc_track_spec(&T, &c, VINE_TRACK_EXACT, &S) == VINE_OK && S.horizon == 1, "H = 1");
        c = config(1, 2, VINE_MPC_MAX_HORIZON);
        expect(vine_mpc_track_spec(&T, &c, VINE_TRACK_LINEAR, &S) == VINE_OK && S.horizon == VINE_MPC_MAX_HORIZON, "H = the largest");
    }

    // refused by name
    {
        VineEnvTargetSpec T = plant_spec(VINE_TARGET_PIPE);
        VineMpcConfig c = config(5, 14, 12);
        expect(vine_mpc_track_spec(nullptr, &c, 0, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_track_spec"), "spec(NULL plant spec)");
        expect(vine_mpc_track_spec(&T, nullptr, 0, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_track_spec"), "spec(NULL cfg)");
        expect(vine_mpc_track_spec(&T, &c, 0, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_track_spec"), "spec(NULL out)");
        VineEnvTargetSpec bad = T;
        bad.checked = 0u;
        expect(refused_spec(&bad, &c, 0, "was not filled by vine_env_target_spec"), "an unchecked plant spec");
        bad = T;
        bad.abi_version = 9;
        expect(refused_spec(&bad, &c, 0, "VineEnvTargetSpec.abi_version mismatch"), "the plant spec's abi");
        bad = T;
        bad.mode = 3;
        expect(refused_spec(&bad, &c, 0, "mode is not a mode of this library"), "the plant spec's mode");
        VineMpcConfig cb = c;
        cb.abi_version = 9;
        expect(refused_spec(&T, &cb, 0, "VineMpcConfig.abi_version mismatch"), "the config's abi");
        expect(refused_spec(&T, &c, 3, "path 3 is not exact (0), linear (1) or held (2)"), "path 3");
        expect(refused_spec(&T, &c, -1, "path -1 is not exact (0), linear (1) or held (2)"), "path -1");
        cb = config(5, 14, 0);
        expect(refused_spec(&T, &cb, 0, "needs 1 <= horizon <= VINE_MPC_MAX_HORIZON"), "H = 0");
        cb = config(5, 14, VINE_MPC_MAX_HORIZON + 1);
        expect(refused_spec(&T, &cb, 0, "needs 1 <= horizon <= VINE_MPC_MAX_HORIZON"), "H = 65");
        cb = config(0, 14, 12);
        expect(refused_spec(&T, &cb, 0, "num_plants must be at least 1"), "M = 0");
        cb = config(5, 1, 12);
        expect(refused_spec(&T, &cb, 0, "samples must be at least 2"), "K = 1");
        cb = config(1 << 20, 1 << 12, 12);
        expect(refused_spec(&T, &cb, 0, "does not fit an int32"), "M * K");
    }

    // the launches' refusals, with a stand-in handle
    const VineEnvTargetSpec T = plant_spec(VINE_TARGET_PIPE);
    const VineMpcConfig c = config(5, 14, 12);
    expect(vine_mpc_track_spec(&T, &c, VINE_TRACK_EXACT, &S) == VINE_OK, "a pipe spec for the launches");
    VineHandleInfo info;
    memset(&info, 0, sizeof info);
    info.n = 5;
    info.flags = VINE_FLAG_CREATE_PIPE;
    VineHandle* h = reinterpret_cast<VineHandle*>(&info);
#define PLAN(handle, spec, a0, a1, a2, a3, a4, a5) vine_mpc_track_plan(handle, spec, a0, a1, a2, a3, a4, a5, nullptr)
#define NODE(handle, spec, a0, a1, a2, a3) vine_mpc_track_scheduled(handle, spec, a0, a1, a2, a3, nullptr)
    expect(PLAN(nullptr, &S, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_track_plan"), "plan(NULL handle)");
    expect(PLAN(h, nullptr, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_track_plan"), "plan(NULL spec)");
    expect(PLAN(h, &S, nullptr, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "plan(NULL reset)");
    expect(PLAN(h, &S, w, nullptr, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "plan(NULL fresh)");
    expect(PLAN(h, &S, w, u8, nullptr, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "plan(NULL table)");
    expect(PLAN(h, &S, w, u8, p, nullptr, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "plan(NULL motion)");
    expect(PLAN(h, &S, w, u8, p, p, nullptr, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "plan(NULL path)");
    expect(PLAN(h, &S, w, u8, p, p, p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "plan(NULL live)");
    VineMpcTrackSpec bad = S;
    bad.checked = 0u;
    expect(PLAN(h, &bad, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "was not filled by vine_mpc_track_spec"), "plan: unchecked");
    expect(NODE(h, &bad, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "was not filled by vine_mpc_track_spec"), "node: unchecked");
    bad = S;
    bad.abi_version = 7;
    expect(PLAN(h, &bad, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "VineMpcTrackSpec.abi_version mismatch"), "plan: abi");
    expect(NODE(h, &bad, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "VineMpcTrackSpec.abi_version mismatch"), "node: abi");
    bad = S;
    bad.horizon = 0;
    expect(PLAN(h, &bad, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "lies outside what vine_mpc_track_spec fills"), "plan: H = 0");
    bad = S;
    bad.samples = 0;
    expect(NODE(h, &bad, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "lies outside what vine_mpc_track_spec fills"), "node: K = 0");
    // the handles' sizes
    info.n = 5 * 14;
    expect(PLAN(h, &S, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "the plant handle has 70 envs, not num_plants = 5"), "plan: M");
    info.n = 5;
    expect(NODE(h, &S, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "the model handle has 5 envs, not num_plants * samples = 5 * 14"),
           "node: M * K");
    // the mode against the handle's obstacle flags
    info.flags = VINE_FLAG_CREATE_SHELF;
    expect(PLAN(h, &S, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "mode is not that of the handle's obstacle flags"), "plan: mode");
    info.n = 5 * 14;
    info.flags = 0u;
    expect(NODE(h, &S, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "mode is not that of the handle's obstacle flags"), "node: mode");
    // the node's null pointers, and a handle's own refusal passed on
    info.flags = VINE_FLAG_CREATE_PIPE;
    expect(NODE(nullptr, &S, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_track_scheduled"), "node(NULL handle)");
    expect(NODE(h, nullptr, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "node(NULL spec)");
    expect(NODE(h, &S, nullptr, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "node(NULL window)");
    expect(NODE(h, &S, w, nullptr, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "node(NULL alive)");
    expect(NODE(h, &S, w, u8, nullptr, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "node(NULL path)");
    expect(NODE(h, &S, w, u8, p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "node(NULL live)");
    info.n = 0;
    expect(PLAN(h, &S, w, u8, p, p, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"), "plan: the handle's refusal passed on");
    expect(NODE(h, &S, w, u8, p, u8) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"), "node: the handle's refusal passed on");

    if (failures) return 1;
    printf("mpc track host check ok\n");
    return 0;
}
