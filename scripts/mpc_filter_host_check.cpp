// mpc_filter_host_check.cpp — the host-side entry points of csrc/vine_mpc_filter.hip on their refusal paths, as a stand-alone
// program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_filter_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc_filter.hip -o build/mpc_filter_host_check
//   ./build/mpc_filter_host_check
//
// The functions vine_mpc_filter.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, as
// scripts/mpc_observe_host_check.cpp does: a stand-in handle is a VineHandleInfo of this program's own making, which lets
// every refusal of a pair of handles be walked without a device.  Exit status 0 and "mpc filter host check ok" when every
// refusal is what include/vine_mpc_filter.h says.
#include <cstdio>
#include <cstring>

#include "../include/vine_mpc_filter.h"
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
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_err);
    }
}

static VineHandleInfo handle(int n) {
    VineHandleInfo info;
    memset(&info, 0, sizeof info);
    info.n = n;
    info.max_len = 100;
    info.delay = 1;
    return info;
}
static VineHandle* as_handle(VineHandleInfo& info) { return reinterpret_cast<VineHandle*>(&info); }

alignas(16) static char buf[128];
static float* const p = reinterpret_cast<float*>(buf + 16);
static float* const odd4 = reinterpret_cast<float*>(buf + 20);      // 4-byte aligned only
static int64_t* const w = reinterpret_cast<int64_t*>(buf + 32);
static int32_t* const i32 = reinterpret_cast<int32_t*>(buf + 64);
static uint8_t* const u8 = reinterpret_cast<uint8_t*>(buf + 96);

static int pin(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* c, bool null_args = false, float* actions = p,
               const float* log = p) {
    if (null_args)
        return vine_mpc_filter_pin(plant, predictor, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr);
    return vine_mpc_filter_pin(plant, predictor, c, p, w, p, w, log, i32, u8, actions, p, w, w, nullptr);
}
static int correct(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* c, bool null_args = false) {
    if (null_args)
        return vine_mpc_filter_correct(plant, predictor, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr);
    return vine_mpc_filter_correct(plant, predictor, c, p, p, p, i32, u8, p, w, p, nullptr);
}

static VineMpcObserveConfig good() {
    VineMpcObserveConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_MPC_OBSERVE_ABI_VERSION;
    c.num_plants = 3;
    c.catchup = 2;
    c.compensate = 1;
    return c;
}

template <class Change>
static void refused_everywhere(const char* word, Change change) {
    VineMpcObserveConfig c = good();
    change(c);
    VineHandleInfo a = handle(3), b = handle(3);
    expect(pin(as_handle(a), as_handle(b), &c) == VINE_ERR_INVALID_ARG && strstr(g_err, word), word);
    expect(correct(as_handle(a), as_handle(b), &c) == VINE_ERR_INVALID_ARG && strstr(g_err, word), word);
}

// a predictor that differs from the plant in one respect
template <class Change>
static void predictor_refused(int code, const char* word, Change change) {
    const VineMpcObserveConfig c = good();
    VineHandleInfo a = handle(3), b = handle(3);
    change(b);
    expect(pin(as_handle(a), as_handle(b), &c) == code && strstr(g_err, word), word);
    expect(correct(as_handle(a), as_handle(b), &c) == code && strstr(g_err, word), word);
}

int main() {
    expect(vine_mpc_filter_abi_version() == VINE_MPC_FILTER_ABI_VERSION, "abi version");

    typedef VineMpcObserveConfig C;
    refused_everywhere("mpc filter: VineMpcObserveConfig.abi_version", [](C& c) { c.abi_version = 7; });
    refused_everywhere("mpc filter: num_plants", [](C& c) { c.num_plants = 0; });

    VineMpcObserveConfig c = good();
    VineHandleInfo a = handle(3), b = handle(3);
    VineHandle *ha = as_handle(a), *hb = as_handle(b);
    expect(pin(ha, hb, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc filter: the observe config is NULL"), "pin(NULL config)");
    expect(correct(ha, hb, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc filter: the observe config is NULL"),
           "correct(NULL config)");
    expect(pin(ha, hb, &c, true) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_filter_pin"), "pin(NULL)");
    expect(correct(ha, hb, &c, true) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_filter_correct"),
           "correct(NULL)");
    expect(pin(nullptr, hb, &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "pin(NULL plant)");
    expect(correct(ha, nullptr, &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "correct(NULL predictor)");

    // past the null checks: misaligned buffers, one handle twice
    expect(pin(ha, hb, &c, false, odd4) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"), "pin(misaligned actions)");
    expect(pin(ha, hb, &c, false, p, odd4) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"), "pin(misaligned act_log)");
    expect(pin(ha, ha, &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "two handles"), "pin(one handle twice)");
    expect(correct(ha, ha, &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "two handles"), "correct(one handle twice)");

    // the handles: a refusal of the handle itself is passed on; then every pair the observe pin would refuse
    VineHandleInfo dead = handle(0), four = handle(4);
    expect(pin(as_handle(dead), hb, &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"), "pin(plant refusal passed on)");
    expect(correct(ha, as_handle(dead), &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "correct(predictor refusal passed on)");
    expect(pin(as_handle(four), hb, &c) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc filter: the plant handle does not have num_plants envs"),
           "pin(plant env count)");
    expect(correct(as_handle(four), hb, &c) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "mpc filter: the plant handle does not have num_plants envs"),
           "correct(plant env count)");
    predictor_refused(VINE_ERR_INVALID_ARG, "mpc filter: the predictor handle has 4 envs, not num_plants = 3",
                      [](VineHandleInfo& b) { b.n = 4; });
    predictor_refused(VINE_ERR_INVALID_ARG, "mpc filter: the predictor handle sits on another device", [](VineHandleInfo& b) { b.device = 1; });
    predictor_refused(VINE_ERR_UNSUPPORTED, "vine_randomize", [](VineHandleInfo& b) { b.flags |= VINE_FLAG_VINE_RANDOMIZE; });
    predictor_refused(VINE_ERR_UNSUPPORTED, "CREATE_SHELF / CREATE_PIPE", [](VineHandleInfo& b) { b.flags |= VINE_FLAG_CREATE_PIPE; });
    predictor_refused(VINE_ERR_UNSUPPORTED, "CREATE_SHELF / CREATE_PIPE", [](VineHandleInfo& b) { b.flags |= VINE_FLAG_CREATE_SHELF; });
    predictor_refused(VINE_ERR_INVALID_ARG, "max_episode_length", [](VineHandleInfo& b) { b.max_len = 99; });

    if (failures) return 1;
    printf("mpc filter host check ok\n");
    return 0;
}
