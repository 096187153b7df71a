// mpc_host_check.cpp — the host-side entry points of csrc/vine_mpc.hip on their refusal paths, as a stand-alone program for
// a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc.hip -o build/mpc_host_check
//   ./build/mpc_host_check
//
// The three functions vine_mpc.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, so that the unit is
// checked alone.  Exit status 0 and "mpc host check ok" when every refusal is what include/vine_mpc.h says.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/vine_mpc.h"

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

template <class Change>
static void refused_everywhere(const char* word, Change change) {
    VineMpcConfig c;
    vine_mpc_config_default(&c);
    c.num_plants = 3;
    change(c);
    VineHandle* none = nullptr;
    const int rc[3] = {
        vine_mpc_fork(none, none, &c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr),
        vine_mpc_scheduled(none, &c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
        vine_mpc_update(none, &c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)};
    for (int i = 0; i < 3; ++i) expect(rc[i] == VINE_ERR_INVALID_ARG, word);
    expect(strstr(g_err, word) != nullptr, word);
}

int main() {
    VineMpcConfig c;
    memset(&c, 0xff, sizeof c);
    expect(vine_mpc_config_default(nullptr) == VINE_ERR_INVALID_ARG, "default(NULL)");
    expect(vine_mpc_config_default(&c) == VINE_OK, "default");
    expect(c.abi_version == VINE_MPC_ABI_VERSION && c.num_plants == 0 && c.samples == 256 && c.horizon == 20 && c.lambda == 0.05 &&
               c.sigma[0] == 0.5f && c.sigma[1] == 0.5f && c.seed == 0,
           "default values");
    expect(vine_mpc_config_size() == (int)sizeof(VineMpcConfig) && sizeof(VineMpcConfig) == 40, "size");

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    refused_everywhere("abi_version", [](VineMpcConfig& c) { c.abi_version = 7; });
    refused_everywhere("num_plants", [](VineMpcConfig& c) { c.num_plants = 0; });
    refused_everywhere("samples", [](VineMpcConfig& c) { c.samples = 1; });
    refused_everywhere("num_plants * samples", [](VineMpcConfig& c) { c.num_plants = 1 << 20; c.samples = 1 << 20; });
    refused_everywhere("horizon", [](VineMpcConfig& c) { c.horizon = 0; });
    refused_everywhere("horizon", [](VineMpcConfig& c) { c.horizon = VINE_MPC_MAX_HORIZON + 1; });
    refused_everywhere("lambda", [](VineMpcConfig& c) { c.lambda = 0.0; });
    refused_everywhere("lambda", [=](VineMpcConfig& c) { c.lambda = inf; });
    refused_everywhere("lambda", [=](VineMpcConfig& c) { c.lambda = nan; });
    refused_everywhere("sigma", [](VineMpcConfig& c) { c.sigma[0] = -1.0f; });
    refused_everywhere("sigma", [=](VineMpcConfig& c) { c.sigma[1] = nan; });
    refused_everywhere("sigma", [=](VineMpcConfig& c) { c.sigma[1] = inf; });
    refused_everywhere("null argument", [](VineMpcConfig&) {});

    VineHandle* none = nullptr;
    expect(vine_mpc_fork(none, none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "config is NULL"), "fork(NULL config)");
    expect(vine_mpc_scheduled(none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
               VINE_ERR_INVALID_ARG, "scheduled(NULL config)");
    expect(vine_mpc_update(none, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
               VINE_ERR_INVALID_ARG, "update(NULL config)");

    // past the null checks: misaligned buffers, then the (stand-in) handle's own refusal
    vine_mpc_config_default(&c);
    c.num_plants = 2;
    alignas(8) char buf[64];
    VineHandle* h = reinterpret_cast<VineHandle*>(buf);
    VineHandle* h2 = reinterpret_cast<VineHandle*>(buf + 8);
    void* p = buf + 16;
    void* odd = buf + 20;
    expect(vine_mpc_fork(h, h2, &c, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (float*)odd, (float*)p, (int64_t*)p, (int64_t*)p,
                         (double*)p, (uint8_t*)p, (int64_t*)p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "fork(misaligned actions)");
    expect(vine_mpc_fork(h, h, &c, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (int64_t*)p,
                         (double*)p, (uint8_t*)p, (int64_t*)p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "two handles"),
           "fork(plant == model)");
    expect(vine_mpc_scheduled(h, &c, (float*)p, (int64_t*)p, (int64_t*)p, (float*)odd, (float*)p, (int64_t*)p, (double*)p,
                              (uint8_t*)p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "scheduled(misaligned actions)");
    expect(vine_mpc_update(h, &c, (double*)p, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (float*)odd, nullptr, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"), "update(misaligned plant_actions)");
    expect(vine_mpc_update(h, &c, (double*)p, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (float*)p, nullptr, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"), "update(handle refusal passed on)");

    if (failures) return 1;
    printf("mpc host check ok\n");
    return 0;
}
