// mpc_noise_host_check.cpp — the host-side entry points of csrc/vine_mpc_noise.hip on their refusal paths, as a stand-alone
// program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_noise_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc_noise.hip -o build/mpc_noise_host_check
//   ./build/mpc_noise_host_check
//
// The three functions vine_mpc_noise.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, so that the unit is
// checked alone.  Exit status 0 and "mpc noise host check ok" when every refusal is what include/vine_mpc_noise.h says.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/vine_mpc_noise.h"

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

// The base configuration of include/vine_mpc.h with three plants and sigma (0.5, 0.5).
static VineMpcConfig base() {
    VineMpcConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_MPC_ABI_VERSION;
    c.num_plants = 3;
    c.samples = 256;
    c.horizon = 20;
    c.lambda = 0.05;
    c.sigma[0] = c.sigma[1] = 0.5f;
    return c;
}

template <class Change>
static void refused_everywhere(const char* word, Change change) {
    VineMpcConfig c = base();
    VineMpcNoiseConfig n;
    vine_mpc_noise_config_default(&n);
    change(c, n);
    VineHandle* none = nullptr;
    const int rc[3] = {
        vine_mpc_noise_draw(none, &c, &n, nullptr, nullptr, nullptr),
        vine_mpc_noise_scheduled(none, &c, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
        vine_mpc_noise_update(none, &c, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)};
    for (int i = 0; i < 3; ++i) expect(rc[i] == VINE_ERR_INVALID_ARG, word);
    expect(strstr(g_err, word) != nullptr, word);
}

int main() {
    VineMpcNoiseConfig n;
    memset(&n, 0xff, sizeof n);
    expect(vine_mpc_noise_config_default(nullptr) == VINE_ERR_INVALID_ARG, "default(NULL)");
    expect(vine_mpc_noise_config_default(&n) == VINE_OK, "default");
    expect(n.abi_version == VINE_MPC_NOISE_ABI_VERSION && n.beta[0] == 0.0f && n.beta[1] == 0.0f && n.adapt == 0 && n.rate == 0.2 &&
               n.sigma_min[0] == 0.0f && n.sigma_min[1] == 0.0f && n.sigma_max[0] == FLT_MAX && n.sigma_max[1] == FLT_MAX,
           "default values");
    expect(vine_mpc_noise_config_size() == (int)sizeof(VineMpcNoiseConfig) && sizeof(VineMpcNoiseConfig) == 40, "size");

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const double dnan = std::numeric_limits<double>::quiet_NaN();
    // what vine_mpc.hip refuses of the base configuration, in its words
    refused_everywhere("VineMpcConfig.abi_version", [](VineMpcConfig& c, VineMpcNoiseConfig&) { c.abi_version = 7; });
    refused_everywhere("num_plants", [](VineMpcConfig& c, VineMpcNoiseConfig&) { c.num_plants = 0; });
    refused_everywhere("samples", [](VineMpcConfig& c, VineMpcNoiseConfig&) { c.samples = 1; });
    refused_everywhere("horizon", [](VineMpcConfig& c, VineMpcNoiseConfig&) { c.horizon = VINE_MPC_MAX_HORIZON + 1; });
    refused_everywhere("lambda", [](VineMpcConfig& c, VineMpcNoiseConfig&) { c.lambda = 0.0; });
    refused_everywhere("mpc sigma", [](VineMpcConfig& c, VineMpcNoiseConfig&) { c.sigma[0] = -1.0f; });
    // the noise configuration's own
    refused_everywhere("VineMpcNoiseConfig.abi_version", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.abi_version = 7; });
    refused_everywhere("beta", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.beta[0] = 1.0f; });
    refused_everywhere("beta", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.beta[1] = -0.1f; });
    refused_everywhere("beta", [=](VineMpcConfig&, VineMpcNoiseConfig& n) { n.beta[1] = nan; });
    refused_everywhere("beta", [=](VineMpcConfig&, VineMpcNoiseConfig& n) { n.beta[0] = inf; });
    refused_everywhere("rate", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.adapt = 1; n.rate = 0.0; });
    refused_everywhere("rate", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.adapt = 1; n.rate = 1.5; });
    refused_everywhere("rate", [=](VineMpcConfig&, VineMpcNoiseConfig& n) { n.adapt = 1; n.rate = dnan; });
    refused_everywhere("sigma_min", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.sigma_min[0] = -0.5f; });
    refused_everywhere("sigma_min", [=](VineMpcConfig&, VineMpcNoiseConfig& n) { n.sigma_min[1] = nan; });
    refused_everywhere("sigma_max", [=](VineMpcConfig&, VineMpcNoiseConfig& n) { n.sigma_max[1] = inf; });
    refused_everywhere("sigma_max", [=](VineMpcConfig&, VineMpcNoiseConfig& n) { n.sigma_max[0] = nan; });
    refused_everywhere("sigma_min <= sigma <= sigma_max", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.sigma_min[0] = 0.6f; });
    refused_everywhere("sigma_min <= sigma <= sigma_max", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.sigma_max[1] = 0.4f; });
    // without adapt the rate is not looked at
    refused_everywhere("null argument", [](VineMpcConfig&, VineMpcNoiseConfig& n) { n.rate = 7.0; });
    refused_everywhere("null argument", [](VineMpcConfig&, VineMpcNoiseConfig&) {});

    VineMpcConfig c = base();
    VineHandle* none = nullptr;
    expect(vine_mpc_noise_draw(none, nullptr, &n, nullptr, nullptr, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc config is NULL"),
           "draw(NULL config)");
    expect(vine_mpc_noise_draw(none, &c, nullptr, nullptr, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "mpc noise config is NULL"), "draw(NULL noise config)");
    expect(vine_mpc_noise_scheduled(none, &c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == VINE_ERR_INVALID_ARG,
           "scheduled(NULL noise config)");
    expect(vine_mpc_noise_update(none, &c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr) == VINE_ERR_INVALID_ARG, "update(NULL noise config)");

    // past the null checks: misaligned buffers, then the (stand-in) handle's own refusal
    alignas(8) char buf[64];
    VineHandle* h = reinterpret_cast<VineHandle*>(buf);
    void* p = buf + 16;
    void* odd = buf + 20;
    expect(vine_mpc_noise_draw(h, &c, &n, (int64_t*)p, (float*)odd, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "draw(misaligned eps)");
    expect(vine_mpc_noise_draw(h, &c, &n, (int64_t*)p, (float*)p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "draw(handle refusal passed on)");
    expect(vine_mpc_noise_scheduled(h, &c, &n, (float*)p, (int64_t*)p, (float*)p, (float*)p, (float*)odd, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"), "scheduled(misaligned actions)");
    expect(vine_mpc_noise_scheduled(h, &c, &n, (float*)p, (int64_t*)p, (float*)p, (float*)odd, (float*)p, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"), "scheduled(misaligned sigma_p)");
    expect(vine_mpc_noise_scheduled(h, &c, &n, (float*)p, (int64_t*)p, (float*)p, (float*)p, (float*)p, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"), "scheduled(handle refusal passed on)");
    expect(vine_mpc_noise_update(h, &c, &n, (double*)p, (int64_t*)p, (float*)odd, (float*)p, (float*)p, (int64_t*)p, (float*)p,
                                 (float*)p, nullptr, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "update(misaligned eps)");
    expect(vine_mpc_noise_update(h, &c, &n, (double*)p, (int64_t*)p, (float*)p, (float*)p, (float*)p, (int64_t*)p, (float*)odd,
                                 (float*)p, nullptr, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "update(misaligned plant_actions)");
    expect(vine_mpc_noise_update(h, &c, &n, (double*)p, (int64_t*)p, (float*)p, (float*)p, (float*)p, (int64_t*)p, (float*)p,
                                 (float*)p, nullptr, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "update(handle refusal passed on)");

    if (failures) return 1;
    printf("mpc noise host check ok\n");
    return 0;
}
