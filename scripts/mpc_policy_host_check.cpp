// mpc_policy_host_check.cpp — the host-side entry points of csrc/vine_mpc_policy.hip on their refusal paths, as a stand-alone
// program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_policy_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc_policy.hip -o build/mpc_policy_host_check
//   ./build/mpc_policy_host_check
//
// The functions vine_mpc_policy.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, so that the unit is
// checked alone.  Exit status 0 and "mpc policy host check ok" when every refusal is what include/vine_mpc_policy.h says.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/vine_mpc_policy.h"

static char g_err[256];
extern "C" {
void vine_set_error(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
int vine_handle_info(VineHandle*, void*) {
    vine_set_error("stand-in handle");
    return VINE_ERR_INVALID_ARG;
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

static void good(VineMpcConfig& c, VineMpcPolicyConfig& pc) {
    c.abi_version = VINE_MPC_ABI_VERSION;
    c.num_plants = 2;
    c.samples = 256;
    c.horizon = 3;
    c.lambda = 0.05;
    c.sigma[0] = c.sigma[1] = 0.5f;
    c.seed = 0;
    vine_mpc_policy_config_default(&pc);
    pc.obs_width = 26;
}

static void call_all(const VineMpcConfig* c, const VineMpcPolicyConfig* pc, int rc[4]) {
    VineHandle* none = nullptr;
    rc[0] = vine_mpc_policy_fork(none, none, c, pc, nullptr, 26, nullptr, 26, nullptr, nullptr, nullptr, nullptr, nullptr, 352, nullptr);
    rc[1] = vine_mpc_policy_act(none, c, pc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr);
    rc[2] = vine_mpc_policy_terminal(none, c, pc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr);
    rc[3] = vine_mpc_policy_compose(none, c, pc, nullptr, nullptr, nullptr, nullptr, nullptr);
}

template <class Change>
static void refused_everywhere(const char* word, Change change) {
    VineMpcConfig c;
    VineMpcPolicyConfig pc;
    good(c, pc);
    change(c, pc);
    int rc[4];
    call_all(&c, &pc, rc);
    for (int i = 0; i < 4; ++i) expect(rc[i] == VINE_ERR_INVALID_ARG, word);
    expect(strstr(g_err, word) != nullptr, word);
}

int main() {
    VineMpcPolicyConfig pc;
    memset(&pc, 0xff, sizeof pc);
    expect(vine_mpc_policy_config_default(nullptr) == VINE_ERR_INVALID_ARG, "default(NULL)");
    expect(vine_mpc_policy_config_default(&pc) == VINE_OK, "default");
    expect(pc.abi_version == VINE_MPC_POLICY_ABI_VERSION && pc.obs_width == 0 && pc.ln_eps == 1e-5f && pc.value_eps == 1e-5f &&
               pc.terminal_value == 0.0, "default values");
    expect(vine_mpc_policy_config_size() == (int)sizeof(VineMpcPolicyConfig) && sizeof(VineMpcPolicyConfig) == 24, "size");

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    typedef VineMpcConfig C;
    typedef VineMpcPolicyConfig P;
    refused_everywhere("VineMpcConfig.abi_version", [](C& c, P&) { c.abi_version = 7; });
    refused_everywhere("VineMpcPolicyConfig.abi_version", [](C&, P& p) { p.abi_version = 7; });
    refused_everywhere("num_plants", [](C& c, P&) { c.num_plants = 0; });
    refused_everywhere("samples", [](C& c, P&) { c.samples = 1; });
    refused_everywhere("num_plants * samples does not fit", [](C& c, P&) { c.num_plants = 1 << 20; c.samples = 1 << 20; });
    refused_everywhere("horizon", [](C& c, P&) { c.horizon = 0; });
    refused_everywhere("horizon", [](C& c, P&) { c.horizon = VINE_MPC_MAX_HORIZON + 1; });
    refused_everywhere("multiple of 512", [](C& c, P&) { c.samples = 255; });
    refused_everywhere("multiple of 512", [](C& c, P&) { c.num_plants = 1; });
    refused_everywhere("obs_width", [](C&, P& p) { p.obs_width = 0; });
    refused_everywhere("obs_width", [](C&, P& p) { p.obs_width = VINE_MAX_OBS + 1; });
    refused_everywhere("ln_eps", [=](C&, P& p) { p.ln_eps = (float)nan; });
    refused_everywhere("ln_eps", [](C&, P& p) { p.ln_eps = -1e-5f; });
    refused_everywhere("value_eps", [=](C&, P& p) { p.value_eps = (float)inf; });
    refused_everywhere("terminal_value", [](C&, P& p) { p.terminal_value = -0.5; });
    refused_everywhere("terminal_value", [=](C&, P& p) { p.terminal_value = inf; });
    refused_everywhere("terminal_value", [=](C&, P& p) { p.terminal_value = nan; });
    refused_everywhere("null argument", [](C&, P&) {});
    refused_everywhere("null argument", [](C& c, P& p) { c.num_plants = 3; c.samples = 512; p.terminal_value = 2.0; });

    VineMpcConfig c;
    good(c, pc);
    int rc[4];
    call_all(nullptr, &pc, rc);
    for (int i = 0; i < 4; ++i) expect(rc[i] == VINE_ERR_INVALID_ARG, "NULL config");
    expect(strstr(g_err, "mpc config is NULL") != nullptr, "NULL config");
    call_all(&c, nullptr, rc);
    for (int i = 0; i < 4; ++i) expect(rc[i] == VINE_ERR_INVALID_ARG, "NULL policy config");
    expect(strstr(g_err, "mpc policy config is NULL") != nullptr, "NULL policy config");

    // past the null checks: widths, misaligned buffers, then the (stand-in) handle's own refusal
    alignas(16) char buf[128];
    VineHandle* h = reinterpret_cast<VineHandle*>(buf);
    VineHandle* h2 = reinterpret_cast<VineHandle*>(buf + 64);
    float* p = reinterpret_cast<float*>(buf + 16);
    float* odd8 = reinterpret_cast<float*>(buf + 24);      // 8-byte aligned only
    float* odd4 = reinterpret_cast<float*>(buf + 20);      // 4-byte aligned only
    expect(vine_mpc_policy_fork(h, h2, &c, &pc, p, 26, p, 14, p, p, p, p, p, 352, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "observation width"), "fork(widths differ)");
    expect(vine_mpc_policy_fork(h, h2, &c, &pc, p, 14, p, 14, p, p, p, p, p, 352, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "observation width"), "fork(widths differ from the configuration's)");
    expect(vine_mpc_policy_fork(h, h2, &c, &pc, p, 26, p, 26, p, odd8, p, p, p, 352, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "16-byte aligned"), "fork(misaligned plant_c)");
    expect(vine_mpc_policy_fork(h, h2, &c, &pc, p, 26, p, 26, p, p, p, p, p, 350, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "16-byte aligned"), "fork(h_op_stride no multiple of 4)");
    expect(vine_mpc_policy_fork(h, h2, &c, &pc, p, 26, p, 26, p, p, p, p, p, 128, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "16-byte aligned"), "fork(h_op_stride below 256)");
    expect(vine_mpc_policy_fork(h, h, &c, &pc, p, 26, p, 26, p, p, p, p, p, 352, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "two handles"), "fork(one handle twice)");
    expect(vine_mpc_policy_fork(h, h2, &c, &pc, p, 26, p, 26, p, p, p, p, p, 352, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "stand-in handle"), "fork(handle refusal passed on)");
    const int64_t* w = reinterpret_cast<const int64_t*>(p);
    expect(vine_mpc_policy_act(h, &c, &pc, odd8, p, p, w, w, p, p, p, p, p, p, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "16-byte aligned"), "act(misaligned y)");
    expect(vine_mpc_policy_act(h, &c, &pc, p, p, p, w, w, p, p, odd4, p, p, p, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "8-byte aligned"), "act(misaligned actions)");
    expect(vine_mpc_policy_act(h, &c, &pc, p, p, p, w, w, p, p, p, p, p, p, odd4, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "8-byte aligned"), "act(misaligned mu_out)");
    expect(vine_mpc_policy_act(h, &c, &pc, p, p, p, w, w, p, p, p, p, p, p, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "stand-in handle"), "act(handle refusal passed on, mu_out NULL allowed)");
    double* dp = reinterpret_cast<double*>(p);
    uint8_t* bp = reinterpret_cast<uint8_t*>(p);
    expect(vine_mpc_policy_terminal(h, &c, &pc, p, p, p, dp, nullptr, w, dp, bp, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "both or neither"), "terminal(one statistic only)");
    expect(vine_mpc_policy_terminal(h, &c, &pc, p, odd8, p, dp, dp, w, dp, bp, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "16-byte aligned"), "terminal(misaligned hw)");
    expect(vine_mpc_policy_terminal(h, &c, &pc, p, p, p, nullptr, nullptr, w, dp, bp, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "stand-in handle"), "terminal(handle refusal passed on, no statistics allowed)");
    expect(vine_mpc_policy_compose(h, &c, &pc, p, w, odd4, p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "compose(misaligned plant_actions)");
    expect(vine_mpc_policy_compose(h, &c, &pc, p, w, p, p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "compose(handle refusal passed on)");

    if (failures) return 1;
    printf("mpc policy host check ok\n");
    return 0;
}
