// mpc_adapt_host_check.cpp — the host-side entry points of csrc/vine_mpc_adapt.hip on their refusal paths, as a stand-alone
// program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_adapt_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc_adapt.hip -o build/mpc_adapt_host_check
//   ./build/mpc_adapt_host_check
//
// The three functions vine_mpc_adapt.hip needs of vine_hip.hip (vine_observer.h) are stood in for here, so that the unit is
// checked alone.  Exit status 0 and "mpc adapt host check ok" when every refusal is what include/vine_mpc_adapt.h says.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/vine_env_params.h"
#include "../include/vine_mpc_adapt.h"

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

static void good(VineMpcAdaptConfig& c) {
    vine_mpc_adapt_config_default(&c);
    c.num_plants = 3;
    c.num_dims = 1;
    c.dims[0] = VineMpcAdaptDim{VP_DAMPING, 1, 0.005, 0.1, 0.001};
}

static void call_all(const VineMpcAdaptConfig* c, int rc[5]) {
    VineHandle* none = nullptr;
    rc[0] = vine_mpc_adapt_anchor(none, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr);
    rc[1] = vine_mpc_adapt_trace(none, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr);
    rc[2] = vine_mpc_adapt_pin(none, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr);
    rc[3] = vine_mpc_adapt_scheduled(none, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    rc[4] = vine_mpc_adapt_estimate(none, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr);
}

template <class Change>
static void refused_everywhere(const char* word, Change change, int want = VINE_ERR_INVALID_ARG) {
    VineMpcAdaptConfig c;
    good(c);
    change(c);
    int rc[5];
    call_all(&c, rc);
    for (int i = 0; i < 5; ++i) expect(rc[i] == want, word);
    expect(strstr(g_err, word) != nullptr, word);
}

int main() {
    VineMpcAdaptConfig c;
    memset(&c, 0xff, sizeof c);
    expect(vine_mpc_adapt_config_default(nullptr) == VINE_ERR_INVALID_ARG, "default(NULL)");
    expect(vine_mpc_adapt_config_default(&c) == VINE_OK, "default");
    expect(c.abi_version == VINE_MPC_ADAPT_ABI_VERSION && c.num_plants == 0 && c.samples == 256 && c.window == 8 && c.every == 8 &&
               c.num_dims == 0 && c.min_steps == 4 && c.forget_on_reset == 0 && c.temperature == 0.1 && c.rate == 0.5 &&
               c.seed == 0 && c.weights[0] == 1.0f && c.weights[5] == 1.0f && c.weights[6] == 0.0f && c.weights[11] == 0.0f &&
               c.base_rows[0] == 0.0f && c.dims[7].num_rows == 0,
           "default values");
    expect(vine_mpc_adapt_config_size() == (int)sizeof(VineMpcAdaptConfig) && sizeof(VineMpcAdaptConfig) == 440 &&
               sizeof(VineMpcAdaptDim) == 32, "size");

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    typedef VineMpcAdaptConfig C;
    refused_everywhere("abi_version", [](C& c) { c.abi_version = 7; });
    refused_everywhere("num_plants", [](C& c) { c.num_plants = 0; });
    refused_everywhere("samples", [](C& c) { c.samples = 1; });
    refused_everywhere("num_plants * samples", [](C& c) { c.num_plants = 1 << 20; c.samples = 1 << 20; });
    refused_everywhere("window", [](C& c) { c.window = 0; });
    refused_everywhere("window", [](C& c) { c.window = VINE_MPC_ADAPT_MAX_WINDOW + 1; c.every = 64; });
    refused_everywhere("window <= every", [](C& c) { c.every = 7; });
    refused_everywhere("num_dims", [](C& c) { c.num_dims = 0; });
    refused_everywhere("num_dims", [](C& c) { c.num_dims = VINE_MPC_ADAPT_MAX_DIMS + 1; });
    refused_everywhere("min_steps", [](C& c) { c.min_steps = 0; });
    refused_everywhere("min_steps", [](C& c) { c.min_steps = 9; });
    refused_everywhere("forget_on_reset", [](C& c) { c.forget_on_reset = -1; });
    refused_everywhere("temperature", [](C& c) { c.temperature = 0.0; });
    refused_everywhere("temperature", [=](C& c) { c.temperature = inf; });
    refused_everywhere("temperature", [=](C& c) { c.temperature = nan; });
    refused_everywhere("rate", [](C& c) { c.rate = 0.0; });
    refused_everywhere("rate", [](C& c) { c.rate = 1.0000001; });
    refused_everywhere("rate", [=](C& c) { c.rate = nan; });
    refused_everywhere("weights", [](C& c) { c.weights[11] = -1.0f; });
    refused_everywhere("weights", [=](C& c) { c.weights[0] = (float)nan; });
    refused_everywhere("base_rows", [=](C& c) { c.base_rows[19] = (float)inf; });
    refused_everywhere("ACTION_DELAY", [](C& c) { c.dims[0].first_row = VP_ACTION_DELAY; }, VINE_ERR_UNSUPPORTED);
    refused_everywhere("dims[0]", [](C& c) { c.dims[0].first_row = VP_COUNT; });
    refused_everywhere("dims[0]", [](C& c) { c.dims[0].first_row = -3; });
    refused_everywhere("dims[0]", [](C& c) { c.dims[0].first_row = 0x7fffffff; c.dims[0].num_rows = 5; });
    refused_everywhere("dims[0]", [](C& c) { c.dims[0].num_rows = 0x7fffffff; });
    refused_everywhere("neither one scalar row nor one FPAM vector", [](C& c) { c.dims[0].first_row = VP_FPAM_C0 + 4; c.dims[0].num_rows = 5; });
    refused_everywhere("neither one scalar row nor one FPAM vector", [](C& c) { c.dims[0].first_row = VP_FPAM_K0; });
    refused_everywhere("lo <= hi", [](C& c) { c.dims[0].lo = 0.2; });
    refused_everywhere("lo <= hi", [=](C& c) { c.dims[0].hi = inf; });
    refused_everywhere("lo <= hi", [=](C& c) { c.dims[0].lo = nan; });
    refused_everywhere("std_floor", [](C& c) { c.dims[0].std_floor = -1e-9; });
    refused_everywhere("std_floor", [=](C& c) { c.dims[0].std_floor = nan; });
    refused_everywhere("dims[1]: overlaps", [](C& c) { c.num_dims = 2; c.dims[1] = c.dims[0]; });
    refused_everywhere("dims[7]: overlaps", [](C& c) {
        c.num_dims = 8;
        for (int d = 0; d < 7; ++d) c.dims[d] = VineMpcAdaptDim{d, 1, 0.0, 1.0, 0.0};
        c.dims[7] = VineMpcAdaptDim{VP_RAIL_ACCELERATION, 1, 0.0, 1.0, 0.0};
    });
    refused_everywhere("null argument", [](C&) {});
    // the widest good configuration gets as far as the null checks too: seven scalar rows and one vector, then four vectors
    refused_everywhere("null argument", [](C& c) {
        c.num_dims = 8;
        for (int d = 0; d < 7; ++d) c.dims[d] = VineMpcAdaptDim{d, 1, -1.0, 1.0, 0.0};
        c.dims[7] = VineMpcAdaptDim{VP_FPAM_B0, 5, 0.5, 1.5, 0.1};
    });
    refused_everywhere("null argument", [](C& c) {
        c.num_dims = 4;
        const int first[4] = {VP_FPAM_K0, VP_FPAM_C0, VP_FPAM_b0, VP_FPAM_B0};
        for (int d = 0; d < 4; ++d) c.dims[d] = VineMpcAdaptDim{first[d], 5, 1.0, 1.0, 0.0};
    });

    int rc[5];
    call_all(nullptr, rc);
    for (int i = 0; i < 5; ++i) expect(rc[i] == VINE_ERR_INVALID_ARG, "NULL config");
    expect(strstr(g_err, "config is NULL") != nullptr, "NULL config");

    // past the null checks: misaligned buffers, then the (stand-in) handle's own refusal
    good(c);
    alignas(8) char buf[64];
    VineHandle* h = reinterpret_cast<VineHandle*>(buf);
    void* p = buf + 16;
    void* odd = buf + 20;
    expect(vine_mpc_adapt_pin(h, &c, (double*)p, (double*)p, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (float*)p, (float*)odd,
                              (float*)p, (int64_t*)p, (int64_t*)p, (double*)p, (uint8_t*)p, (int64_t*)p, nullptr) ==
                   VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"), "pin(misaligned actions)");
    expect(vine_mpc_adapt_scheduled(h, &c, (float*)odd, (float*)p, (int32_t*)p, (int64_t*)p, (float*)p, (int64_t*)p, (double*)p,
                                    (uint8_t*)p, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "8-byte aligned"),
           "scheduled(misaligned trace_actions)");
    expect(vine_mpc_adapt_anchor(h, &c, (int64_t*)p, (int64_t*)p, (float*)p, (float*)p, (float*)p, (int64_t*)p, (int64_t*)p,
                                 (int32_t*)p, (uint8_t*)p, (uint8_t*)p, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "stand-in handle"), "anchor(handle refusal passed on)");
    expect(vine_mpc_adapt_trace(h, &c, (float*)p, (int64_t*)p, (float*)p, (int64_t*)p, (float*)p, (float*)p, (int32_t*)p,
                                (uint8_t*)p, (uint8_t*)p, nullptr, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "stand-in handle"), "trace(handle refusal passed on, returns NULL allowed)");
    expect(vine_mpc_adapt_pin(h, &c, (double*)p, (double*)p, (int64_t*)p, (float*)p, (float*)p, (int64_t*)p, (float*)p, (float*)p,
                              (float*)p, (int64_t*)p, (int64_t*)p, (double*)p, (uint8_t*)p, (int64_t*)p, nullptr) ==
                   VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"), "pin(handle refusal passed on)");
    expect(vine_mpc_adapt_estimate(h, &c, (double*)p, (int32_t*)p, (uint8_t*)p, (double*)p, (double*)p, (double*)p, (double*)p,
                                   (int64_t*)p, nullptr, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "stand-in handle"),
           "estimate(handle refusal passed on, weights NULL allowed)");

    if (failures) return 1;
    printf("mpc adapt host check ok\n");
    return 0;
}
