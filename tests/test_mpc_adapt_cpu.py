"""MPC_ADAPT without a GPU: the C ABI of include/vine_mpc_adapt.h against its ctypes mirror, every refusal of the library and
every ``ConfigError`` of ``adapt_config`` by name, the build plumbing of the twelfth unit, the numpy statement of the estimate
(``mpc_adapt.estimate``) on hand-made errors, and the candidates' deviate under its own purpose word."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_sensor, mpc, mpc_adapt
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_ROW = np.arange(abi.VP_COUNT, dtype=np.float32) + 1.0


def _header():
    return open(os.path.join(REPO, "include", "vine_mpc_adapt.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


def _acfg(lib, dims=((abi.VP_DAMPING, 1, 0.005, 0.1, 0.001),), **over):
    c = abi.VineMpcAdaptConfig()
    assert lib.vine_mpc_adapt_config_default(c) == abi.OK
    c.num_plants, c.num_dims = 3, len(dims)
    for d, (first, count, lo, hi, floor) in enumerate(dims):
        c.dims[d].first_row, c.dims[d].num_rows, c.dims[d].lo, c.dims[d].hi, c.dims[d].std_floor = first, count, lo, hi, floor
    for k, v in over.items():
        if k == "weights":
            for i, x in enumerate(v):
                c.weights[i] = x
        elif k == "base_rows":
            for i, x in enumerate(v):
                c.base_rows[i] = x
        else:
            setattr(c, k, v)
    return c


ENTRY_POINTS = (("vine_mpc_adapt_anchor", 1, 11), ("vine_mpc_adapt_trace", 1, 11), ("vine_mpc_adapt_pin", 1, 15),
                ("vine_mpc_adapt_scheduled", 1, 9), ("vine_mpc_adapt_estimate", 1, 10))


def _entry_points(lib, cfg):
    return [(getattr(lib, name), (None,) * handles + (cfg,) + (None,) * pointers) for name, handles, pointers in ENTRY_POINTS]


# --------------------------------------------------------------------------------------------------------------- ABI
def test_adapt_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_mpc_adapt_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.MPC_ADAPT_PROTOTYPES) and len(names) == 7
    for name in names:
        assert hasattr(hip_lib, name), name
    assert C.sizeof(abi.VineMpcAdaptDim) == 8 + 3 * 8
    assert hip_lib.vine_mpc_adapt_config_size() == C.sizeof(abi.VineMpcAdaptConfig) == 32 + 24 + 48 + 80 + 8 * 32
    for struct, mirror in (("VineMpcAdaptDim", abi.VineMpcAdaptDim), ("VineMpcAdaptConfig", abi.VineMpcAdaptConfig)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
        fields = re.findall(r"^\s+(?:int32_t|float|double|uint64_t|VineMpcAdaptDim)\s+([a-z_]+)(?:\[\w+\])?;", body, re.M)
        assert fields == [n for n, _ in mirror._fields_], struct
    for macro, value in (("ABI_VERSION", abi.MPC_ADAPT_ABI_VERSION), ("MAX_WINDOW", abi.MPC_ADAPT_MAX_WINDOW),
                         ("MAX_DIMS", abi.MPC_ADAPT_MAX_DIMS), ("FIELDS", abi.MPC_ADAPT_FIELDS),
                         ("BASE_ROWS", abi.MPC_ADAPT_BASE_ROWS), ("RNG", abi.MPC_ADAPT_RNG)):
        assert int(re.search(r"#define VINE_MPC_ADAPT_%s (\d+)" % macro, text).group(1)) == value
    assert abi.MPC_ADAPT_BASE_ROWS == abi.VP_COUNT - abi.VP_FPAM_K0 and abi.MPC_ADAPT_FIELDS == len(mpc_adapt.FIELD_NAMES)
    # the purpose word is nobody else's: the next free one behind the controller's noise
    assert abi.MPC_ADAPT_RNG == abi.MPC_RNG_NOISE + 1 == 9
    assert abi.MPC_ADAPT_RNG not in (abi.SENSOR_RNG_NOISE, abi.SENSOR_RNG_HOLD, abi.MPC_RNG_NOISE)
    for name, handles, pointers in ENTRY_POINTS:
        decl = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_ADAPT_PROTOTYPES[name][1]) == handles + 1 + pointers, name      # (the stream counts as a pointer)
    assert "vine_mpc_adapt" not in open(os.path.join(REPO, "include", "vine.h")).read()
    assert "vine_mpc_adapt" not in open(os.path.join(REPO, "include", "vine_mpc.h")).read()
    assert not set(abi.MPC_ADAPT_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.MPC_PROTOTYPES))


def test_adapt_build_plumbing():
    assert native.LIB_UNITS == native.ALL_UNITS + (native.SRC_MPC_ADAPT,) and len(native.LIB_UNITS) == 12
    assert len(native.ALL_UNITS) == 11 and native.SRC_MPC_ADAPT not in native.ALL_UNITS
    assert os.path.basename(native.SRC_MPC_ADAPT) == "vine_mpc_adapt.hip" and os.path.exists(native.SRC_MPC_ADAPT)
    deps = [os.path.basename(d) for d in native.DEPS]
    for name in ("vine_mpc_adapt.hip", "vine_mpc_adapt.h", "vine_mpc_shared.h", "vine_mpc.h", "vine_task_shared.h"):
        assert name in deps, name
    for src in (native.SRC_MPC, native.SRC_MPC_ADAPT):       # both units include the shared statement of the copy and the ring
        assert any(d.endswith("vine_mpc_shared.h") for d in native._SOURCE_HEADERS[src]), src
        text = open(src).read()
        assert '#include "vine_mpc_shared.h"' in text
        assert text.index('#include "vine_task_shared.h"') < text.index('#include "vine_mpc_shared.h"')
    assert any(d.endswith("vine_mpc_adapt.h") for d in native._SOURCE_HEADERS[native.SRC_MPC_ADAPT])
    assert native._SOURCE_FLAGS[native.SRC_MPC_ADAPT] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_MPC_ADAPT)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast")
    src = open(native.SRC_MPC_ADAPT).read()
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")
    before = src[:src.index('#include "vine_task_shared.h"')]
    assert before.rstrip().endswith("#pragma clang fp contract(fast)")          # the ring holds the step kernels' bits
    assert "atomic" not in re.sub(r"//.*", "", src)
    shared = open(os.path.join(os.path.dirname(native.SRC_MPC), "vine_mpc_shared.h")).read()
    # stated once: the fork no longer spells the copy or the ring out
    mpc_src = open(native.SRC_MPC).read()
    assert "task_new_command<false>" in shared and "task_new_command<false>" not in mpc_src
    assert "task_new_command<false>" not in src and "mpc_rebuild_ring(" in mpc_src and "mpc_rebuild_ring(" in src
    assert "MPC_COPY_COLUMN(" in mpc_src and "MPC_COPY_COLUMN(" in src and "#define MPC_COPY_COLUMN(" in shared


def test_adapt_defaults(hip_lib):
    c = abi.VineMpcAdaptConfig()
    assert hip_lib.vine_mpc_adapt_config_default(c) == abi.OK
    assert (c.abi_version, c.num_plants, c.samples, c.window, c.every, c.num_dims, c.min_steps, c.forget_on_reset, c.temperature,
            c.rate, c.seed) == (1, 0, 256, 8, 8, 0, 4, 0, 0.1, 0.5, 0)
    assert list(c.weights) == [1.0] * 6 + [0.0] * 6 and not any(c.base_rows)
    assert (c.window, c.every, c.min_steps, c.temperature, c.rate) == tuple(
        mpc_adapt.DEFAULTS[k] for k in ("window", "every", "min_steps", "temperature", "rate"))
    assert c.samples == mpc.DEFAULTS["samples"]
    assert hip_lib.vine_mpc_adapt_config_default(None) == abi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------- the library's refusals
DAMP = (abi.VP_DAMPING, 1, 0.005, 0.1, 0.001)


@pytest.mark.parametrize("over, rc, word", [
    (dict(abi_version=7), abi.ERR_INVALID_ARG, b"abi_version"), (dict(num_plants=0), abi.ERR_INVALID_ARG, b"num_plants"),
    (dict(samples=1), abi.ERR_INVALID_ARG, b"samples"),
    (dict(num_plants=1 << 20, samples=1 << 20), abi.ERR_INVALID_ARG, b"num_plants * samples"),
    (dict(window=0), abi.ERR_INVALID_ARG, b"window"), (dict(window=33, every=40), abi.ERR_INVALID_ARG, b"window"),
    (dict(window=8, every=7), abi.ERR_INVALID_ARG, b"window <= every"), (dict(num_dims=0), abi.ERR_INVALID_ARG, b"num_dims"),
    (dict(num_dims=9), abi.ERR_INVALID_ARG, b"num_dims"), (dict(min_steps=0), abi.ERR_INVALID_ARG, b"min_steps"),
    (dict(min_steps=9), abi.ERR_INVALID_ARG, b"min_steps"), (dict(forget_on_reset=2), abi.ERR_INVALID_ARG, b"forget_on_reset"),
    (dict(temperature=0.0), abi.ERR_INVALID_ARG, b"temperature"),
    (dict(temperature=float("nan")), abi.ERR_INVALID_ARG, b"temperature"),
    (dict(temperature=float("inf")), abi.ERR_INVALID_ARG, b"temperature"), (dict(rate=0.0), abi.ERR_INVALID_ARG, b"rate"),
    (dict(rate=1.5), abi.ERR_INVALID_ARG, b"rate"), (dict(rate=float("nan")), abi.ERR_INVALID_ARG, b"rate"),
    (dict(weights=[-1.0]), abi.ERR_INVALID_ARG, b"weights"), (dict(weights=[1.0, float("inf")]), abi.ERR_INVALID_ARG, b"weights"),
    (dict(base_rows=[float("nan")]), abi.ERR_INVALID_ARG, b"base_rows"),
    (dict(dims=((abi.VP_ACTION_DELAY, 1, 0.0, 4.0, 0.1),)), abi.ERR_UNSUPPORTED, b"ACTION_DELAY"),
    (dict(dims=((abi.VP_COUNT, 1, 0.0, 1.0, 0.1),)), abi.ERR_INVALID_ARG, b"dims[0]"),
    (dict(dims=((-1, 1, 0.0, 1.0, 0.1),)), abi.ERR_INVALID_ARG, b"dims[0]"),
    (dict(dims=((abi.VP_FPAM_K0, 1, 0.5, 1.5, 0.1),)), abi.ERR_INVALID_ARG, b"neither one scalar row nor one FPAM vector"),
    (dict(dims=((abi.VP_FPAM_K0 + 1, 5, 0.5, 1.5, 0.1),)), abi.ERR_INVALID_ARG, b"neither one scalar row nor one FPAM vector"),
    (dict(dims=((abi.VP_DAMPING, 5, 0.5, 1.5, 0.1),)), abi.ERR_INVALID_ARG, b"dims[0]"),
    (dict(dims=(DAMP, (abi.VP_RAIL_P_GAIN, 1, 2.0, 1.0, 0.1))), abi.ERR_INVALID_ARG, b"dims[1]: needs finite lo <= hi"),
    (dict(dims=((abi.VP_DAMPING, 1, 0.0, float("inf"), 0.1),)), abi.ERR_INVALID_ARG, b"lo <= hi"),
    (dict(dims=((abi.VP_DAMPING, 1, 0.0, 1.0, -0.1),)), abi.ERR_INVALID_ARG, b"std_floor"),
    (dict(dims=(DAMP, DAMP)), abi.ERR_INVALID_ARG, b"dims[1]: overlaps"),
    (dict(dims=((abi.VP_FPAM_C0, 5, 0.5, 1.5, 0.1), DAMP, (abi.VP_FPAM_C0, 5, 0.7, 1.3, 0.1))), abi.ERR_INVALID_ARG,
     b"dims[2]: overlaps")])
def test_adapt_refuses_bad_configs(hip_lib, over, rc, word):
    """Validation comes before the handles or any pointer is looked at, so no device is needed to see it."""
    over = dict(over)
    bad = _acfg(hip_lib, dims=over.pop("dims", (DAMP,)), **over)
    for fn, args in _entry_points(hip_lib, bad):
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert fn(*args) == rc
        assert word in hip_lib.vine_last_error(), hip_lib.vine_last_error()


def test_adapt_accepts_every_scalar_row_and_every_fpam_vector_and_refuses_null_pointers(hip_lib):
    dims = tuple((r, 1, 0.0, 1.0, 0.0) for r in range(abi.VP_ACTION_DELAY)) + ((abi.VP_FPAM_B0, 5, 0.5, 1.5, 0.0),)
    assert len(dims) == abi.MPC_ADAPT_MAX_DIMS
    for good in (_acfg(hip_lib), _acfg(hip_lib, dims=dims),
                 _acfg(hip_lib, dims=tuple((r, 5, 1.0, 1.0, 0.0) for r in (abi.VP_FPAM_K0, abi.VP_FPAM_C0, abi.VP_FPAM_b0)))):
        for (fn, args), (name, _, _) in zip(_entry_points(hip_lib, good), ENTRY_POINTS):
            assert fn(*args) == abi.ERR_INVALID_ARG
            assert b"null argument to " + name.encode() in hip_lib.vine_last_error(), hip_lib.vine_last_error()
    for fn, args in _entry_points(hip_lib, None):
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert b"config is NULL" in hip_lib.vine_last_error()


# ------------------------------------------------------------------------------------------------------- adapt_config
GOOD = {"params": {"DAMPING": [0.005, 0.1], "FPAM_K": [0.7, 1.3]}, "window": 6, "every": 8}


def test_adapt_config_fills_the_mirror():
    c, names = mpc_adapt.adapt_config(GOOD, 5, 14, BASE_ROW, seed=(1 << 63) + 5, forget_on_reset=True)
    assert names == ["DAMPING", "FPAM_K"]
    assert (c.abi_version, c.num_plants, c.samples, c.window, c.every, c.num_dims, c.min_steps, c.forget_on_reset,
            c.temperature, c.rate, c.seed) == (abi.MPC_ADAPT_ABI_VERSION, 5, 14, 6, 8, 2, 4, 1, mpc_adapt.DEFAULTS["temperature"],
                                               mpc_adapt.DEFAULTS["rate"], (1 << 63) + 5)
    assert list(c.weights) == [1.0] * 6 + [0.0] * 6
    assert list(c.base_rows) == list(BASE_ROW[abi.VP_FPAM_K0:])
    floor = mpc_adapt.DEFAULTS["floor"]
    assert mpc_adapt.dims_of(c) == [(abi.VP_DAMPING, 1, 0.005, 0.1, floor * (0.1 - 0.005)),
                                    (abi.VP_FPAM_K0, 5, 0.7, 1.3, floor * (1.3 - 0.7))]
    assert c.spread == mpc_adapt.DEFAULTS["spread"]
    small, _ = mpc_adapt.adapt_config({"params": {"DAMPING": [0.01, 0.01]}, "window": 1, "weights": {"qd3": 2.0}}, 1, 2, BASE_ROW)
    assert (small.window, small.every, small.min_steps) == (1, 8, 1)            # min_steps follows a short window
    assert list(small.weights) == [0.0] * 9 + [2.0, 0.0, 0.0]


@pytest.mark.parametrize("change, word", [
    ({"params": {"ACTION_DELAY": [0, 4]}}, "params.ACTION_DELAY is refused: an integer"),
    ({"params": {"CART_MASS": [0.5, 2.0]}}, "params.CART_MASS is refused: it lives in the inertia table"),
    ({"params": {"LINK_MASS": [0.7, 1.4]}}, "params.LINK_MASS is refused: it lives in the inertia table"),
    ({"params": {"TIP_LINK_MASS": [0.7, 1.4]}}, "params.TIP_LINK_MASS is refused: it lives in the inertia table"),
    ({"params": {"NO_SUCH": [0, 1]}}, "unknown parameter 'NO_SUCH'"), ({"params": {}}, "params must be a non-empty mapping"),
    ({"params": [1, 2]}, "params must be a non-empty mapping"), ({"params": {"DAMPING": 0.02}}, "params.DAMPING must be a range"),
    ({"params": {"DAMPING": [0.1, 0.005]}}, "params.DAMPING: lo > hi"),
    ({"params": {"DAMPING": [0.0, float("inf")]}}, "adapt.params.DAMPING"),
    ({"params": {n: [0, 1] for n in ("DAMPING", "SMOOTHING_ALPHA_INFLATE", "SMOOTHING_ALPHA_DEFLATE", "RAIL_VELOCITY_SCALE",
                                     "RAIL_P_GAIN", "RAIL_D_GAIN", "RAIL_ACCELERATION", "FPAM_K", "FPAM_C")}}, "at most 8"),
    ({"window": 0}, "adapt.window"), ({"window": 33}, "adapt.window"), ({"window": 2.5}, "adapt.window"),
    ({"window": 8, "every": 7}, "every = 7 must be at least window = 8"), ({"every": True}, "adapt.every"),
    ({"min_steps": 0}, "adapt.min_steps"), ({"min_steps": 7}, "adapt.min_steps"), ({"temperature": 0.0}, "temperature"),
    ({"temperature": "x"}, "adapt.temperature"), ({"rate": 0.0}, "rate"), ({"rate": 1.01}, "rate"),
    ({"rate": float("nan")}, "adapt.rate"), ({"spread": -0.1}, "spread"), ({"floor": -0.1}, "floor"),
    ({"floor": float("inf")}, "adapt.floor"), ({"weights": {"q6": 1.0}}, "unknown field 'q6'"),
    ({"weights": {"q0": -1.0}}, "weights.q0"), ({"weights": [1.0]}, "weights must be a mapping"), ({"horizon": 3}, "unknown key 'horizon'")])
def test_adapt_config_errors_name_the_key(change, word):
    spec = dict(GOOD)
    spec.update(change)
    with pytest.raises(ConfigError, match=re.escape(word)):
        mpc_adapt.adapt_config(spec, 4, 8, BASE_ROW)


def test_adapt_config_refuses_what_is_no_mapping_and_a_bad_seed():
    with pytest.raises(ConfigError, match="must be a mapping"):
        mpc_adapt.adapt_config("DAMPING", 4, 8, BASE_ROW)
    with pytest.raises(ConfigError, match="seed"):
        mpc_adapt.adapt_config(GOOD, 4, 8, BASE_ROW, seed=-1)
    with pytest.raises(ConfigError, match="samples"):
        mpc_adapt.adapt_config(GOOD, 4, 1, BASE_ROW)
    # every refused name carries its sentence
    assert set(mpc_adapt.REFUSED) == {"ACTION_DELAY"} | set(abi.ENV_INERTIA_NAMES)


# ------------------------------------------------------------------------------------------------- candidates and estimate
M, K, D = 3, 10, 2
DIMS = [(abi.VP_DAMPING, 1, 0.005, 0.1, 0.0005), (abi.VP_FPAM_K0, 5, 0.7, 1.3, 0.004)]
MEAN = np.array([[0.05, 1.0], [0.02, 0.9], [0.09, 1.25]])
STD = np.array([[0.02, 0.1], [0.01, 0.2], [0.03, 0.1]])
PRIOR_MEAN, PRIOR_STD = np.full((M, D), 0.5) * [0.1, 2.0], np.full((M, D), 0.25) * [0.095, 0.6]
PASSES = [0, 7, (1 << 32) + 3]


def _theta():
    return mpc_adapt.candidates(MEAN, STD, DIMS, 1234, K, PASSES)


def _estimate(err, trace_len=(6, 6, 6), ended=(0, 0, 0), **kw):
    args = dict(min_steps=4, temperature=0.1, rate=0.5, forget_on_reset=False)
    args.update(kw)
    return mpc_adapt.estimate(err, _theta(), MEAN, STD, PRIOR_MEAN, PRIOR_STD, trace_len, ended, DIMS, **args)


def test_candidate_zero_is_the_belief_and_the_others_stay_in_range():
    th = _theta()
    assert th.shape == (M, K, D) and np.array_equal(th[:, 0], MEAN)
    lo, hi = np.array([d[2] for d in DIMS]), np.array([d[3] for d in DIMS])
    assert (th >= lo).all() and (th <= hi).all() and (th[2, :, 1] == 1.3).any()      # mean 1.25 + draws: some are clamped
    z = mpc_adapt.deviate(1234, M, K, PASSES, D)
    assert z.dtype == np.float32
    assert np.array_equal(th, np.clip(MEAN[:, None] + z.astype(np.float64) * STD[:, None], lo, hi))
    # a pure function of (seed, p, j, pass, d): another pass or seed, other draws; the same, the same
    assert np.array_equal(th, _theta())
    assert not np.array_equal(th[:, 1:], mpc_adapt.candidates(MEAN, STD, DIMS, 1234, K, [1, 7, (1 << 32) + 3])[:, 1:])
    assert not np.array_equal(th[:, 1:], mpc_adapt.candidates(MEAN, STD, DIMS, 1235, K, PASSES)[:, 1:])
    rows = mpc_adapt.table_rows(th, DIMS, BASE_ROW)
    assert sorted(rows) == [abi.VP_DAMPING] + list(range(abi.VP_FPAM_K0, abi.VP_FPAM_K0 + 5))
    assert np.array_equal(rows[abi.VP_DAMPING], th[..., 0].astype(np.float32))
    assert np.array_equal(rows[abi.VP_FPAM_K0 + 3], (np.float64(BASE_ROW[abi.VP_FPAM_K0 + 3]) * th[..., 1]).astype(np.float32))


def test_deviate_under_purpose_word_9_differs_from_word_8s():
    z9 = mpc_adapt.deviate(99, M, K, 5, D)
    z8 = mpc_adapt.deviate(99, M, K, 5, D, purpose=abi.MPC_RNG_NOISE)
    assert not np.array_equal(z9[:, 1:], z8[:, 1:]) and not z9[:, 0].any()
    # word 8's is the controller's own draw: the same counter words give the same integers there
    raw = mpc.noise_deviate(99, M, K, 5, 1)                                   # [M, K, 1, 2]: counter word 3 = 2 k + a = 0, 1
    assert np.array_equal(z8[:, 1:], (raw[:, 1:, 0].astype(np.float64) * env_sensor.NOISE_SCALE).astype(np.float32))
    big = mpc_adapt.deviate(7, 16, 65, 3, 8)[:, 1:].astype(np.float64)
    assert abs(big.mean()) < 5.0 / np.sqrt(big.size) and abs(big.var() - 1.0) < 5.0 * np.sqrt(1.85 / big.size)


def test_estimate_equal_errors_give_the_plain_mean():
    r = _estimate(np.full(M * K, 3.5))
    th = _theta()
    assert np.array_equal(r["weights"], np.ones((M, K))) and r["estimated"].all() and not r["forgot"].any()
    m = th.sum(axis=1) / K
    v = ((th - m[:, None]) ** 2).sum(axis=1) / K
    assert np.allclose(r["mean"], 0.5 * MEAN + 0.5 * m, rtol=1e-15, atol=0)
    floors = np.array([d[4] for d in DIMS])
    assert np.allclose(r["std"], np.maximum(0.5 * STD + 0.5 * np.sqrt(v), floors), rtol=1e-15, atol=0)


def test_estimate_one_finite_error_gives_that_candidate():
    err = np.full((M, K), np.inf)
    best = [4, 0, 9]
    err[np.arange(M), best] = [2.0, 0.0, 1e-9]
    r = _estimate(err.reshape(-1), rate=1.0)
    th = _theta()
    assert np.array_equal(r["weights"], np.isfinite(err).astype(np.float64))
    assert np.array_equal(r["mean"], th[np.arange(M), best])
    assert np.array_equal(r["std"], np.broadcast_to([d[4] for d in DIMS], (M, D)))    # no spread left: the floor
    half = _estimate(err.reshape(-1))
    assert np.array_equal(half["mean"], 0.5 * MEAN + 0.5 * th[np.arange(M), best])
    # and one error far below the rest does the same through the weights
    err2 = np.full((M, K), 100.0)
    err2[np.arange(M), best] = 1.0
    r2 = _estimate(err2.reshape(-1), rate=1.0, temperature=0.001)
    assert np.allclose(r2["mean"], th[np.arange(M), best], rtol=1e-12, atol=0)


def test_estimate_no_finite_error_or_a_short_trace_leaves_the_belief():
    err = np.random.default_rng(0).uniform(0.0, 1.0, (M, K))
    err[1] = np.inf
    r = _estimate(err.reshape(-1), trace_len=(3, 6, 6))
    assert list(r["estimated"]) == [False, False, True]
    assert np.array_equal(r["mean"][:2], MEAN[:2]) and np.array_equal(r["std"][:2], STD[:2])
    assert not r["weights"][:2].any() and r["weights"][2].max() == 1.0
    assert not np.array_equal(r["mean"][2], MEAN[2])
    assert np.array_equal(r["plan"], np.clip(r["mean"], [d[2] for d in DIMS], [d[3] for d in DIMS]))
    assert _estimate(err.reshape(-1), trace_len=(4, 6, 6))["estimated"][0]          # min_steps itself is enough


def test_estimate_forgets_only_when_asked_and_only_the_plants_whose_episode_ended():
    err = np.random.default_rng(1).uniform(0.0, 1.0, M * K)
    kept = _estimate(err, ended=(0, 1, 0))
    assert kept["estimated"].all() and not kept["forgot"].any()
    r = _estimate(err, ended=(0, 1, 0), trace_len=(6, 2, 6), forget_on_reset=True)
    assert list(r["forgot"]) == [False, True, False] and list(r["estimated"]) == [True, False, True]
    assert np.array_equal(r["mean"][1], PRIOR_MEAN[1]) and np.array_equal(r["std"][1], PRIOR_STD[1]) and not r["weights"][1].any()
    for p in (0, 2):
        assert np.array_equal(r["mean"][p], kept["mean"][p]) and np.array_equal(r["std"][p], kept["std"][p])


def test_score_stops_where_the_trace_stops_and_turns_infinite_on_a_nan_or_an_early_reset():
    W, Kk = 3, 2                                                              # two plants, two candidates each
    rows = np.zeros((2, W, 12), dtype=np.float32)
    states = np.zeros((W, 12, 4), dtype=np.float32)
    states[:, 0, :] = [[1.0, 2.0, 1.0, 1.0], [1.0, 2.0, 1.0, np.nan], [1.0, 2.0, 3.0, 1.0]]
    states[:, 7, :] = 100.0                                                   # a qd: weight 0, not compared
    resets = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]])
    w = [1.0] * 6 + [0.0] * 6
    err, alive = mpc_adapt.score(states, resets, rows, [3, 2], w, Kk)
    # candidate 1 reset at k = 2 < 3: out; candidate 0 reset at k = 3 = trace_len: with the plant; plant 1 compares two steps
    assert np.array_equal(err, [3.0, np.inf, 2.0, np.inf]) and np.array_equal(alive, [1, 0, 1, 0])
    err, alive = mpc_adapt.score(states, resets, rows, [0, 1], [2.0] + [0.0] * 11, Kk)
    assert np.array_equal(err, [0.0, 0.0, 2.0, 2.0]) and alive.all()
