"""ENV_INERTIA without a GPU: the header against its ctypes mirror, the host-only entry points of include/vine_env_inertia.h
against float64 numpy, the inertia-table builder of utils/env_params.py, the mass columns of utils/episodes.py, the files,
the search of utils/sysid.py, and the oracle on the nine mass sets of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = abi.NUM_LINKS


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


@pytest.fixture()
def vcfg(lib):
    c = abi.VineConfig()
    assert lib.vine_config_default(C.byref(c)) == 0
    return c


def composites(cart, m, inertia, L, l, g):
    """The derived rows in float64, the statement of include/vine_env_inertia.h: all arguments are the float32 values the
    library reads, widened exactly; python floats are IEEE doubles and round every operation as the host's C does."""
    cart, L, l, g = float(cart), float(L), float(l), float(g)
    m, inertia = [float(x) for x in m], [float(x) for x in inertia]
    out = np.zeros(abi.VI_COUNT)
    mt = cart
    for i in range(NL):
        mt += m[i]
    out[abi.VI_MTOT] = mt
    for i in range(NL):
        distal = 0.0
        for k in range(i + 1, NL):
            distal += m[k]
        b = m[i] * l + L * distal
        out[abi.VI_B0 + i] = b
        out[abi.VI_GB0 + i] = g * b
        out[abi.VI_ADIAG0 + i] = m[i] * l * l + L * L * distal + inertia[i]
        if i > 0:
            out[abi.VI_AOFF1 + i - 1] = L * b
    return out


def expected_column(vcfg, primary):
    """float32 [VI_COUNT]: the primary values as given and the derived rows rounded once from float64."""
    primary = np.asarray(primary, dtype=np.float32)
    col = composites(primary[0], primary[1:1 + NL], primary[1 + NL:1 + 2 * NL], np.float32(vcfg.link_length),
                     np.float32(vcfg.link_com), np.float32(vcfg.gravity)).astype(np.float32)
    col[:abi.VI_PRIMARY_COUNT] = primary
    return col


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def plants(lib, vcfg, n, seed=0):
    """[VI_COUNT, n] with random primary rows around the configuration's (factors 0.5 .. 2), derived rows zero."""
    rng = np.random.default_rng(seed)
    base = env_params.inertia_config_row(lib, vcfg)
    t = np.zeros((abi.VI_COUNT, n), dtype=np.float32)
    t[:abi.VI_PRIMARY_COUNT] = (base[:abi.VI_PRIMARY_COUNT, None] * rng.uniform(0.5, 2.0, (abi.VI_PRIMARY_COUNT, n))).astype(np.float32)
    return t


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_enum_and_prototypes_equal_the_mirror(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_inertia.h")).read(), flags=re.S)
    body = re.search(r"typedef enum VineEnvInertia \{(.*?)\} VineEnvInertia;", text, flags=re.S).group(1)
    value, enum = -1, {}
    for item in [i.strip() for i in body.split(",") if i.strip()]:
        name, _, v = [x.strip() for x in item.partition("=")]
        value = int(v) if v else value + 1
        enum[name] = value
    mirror = {k: getattr(abi, k) for k in dir(abi) if k.startswith("VI_")}
    assert enum == mirror and enum["VI_COUNT"] == 31 and enum["VI_PRIMARY_COUNT"] == 11
    # 11 primary rows, 20 derived rows, every row exactly once
    spans = [(abi.VI_CART_MASS, 1), (abi.VI_LINK_MASS0, NL), (abi.VI_LINK_INERTIA0, NL), (abi.VI_MTOT, 1), (abi.VI_B0, NL),
             (abi.VI_GB0, NL), (abi.VI_ADIAG0, NL), (abi.VI_AOFF1, NL - 1)]
    assert [r for first, count in spans for r in range(first, first + count)] == list(range(abi.VI_COUNT))
    assert len(abi.ENV_INERTIA_ROW_NAMES) == abi.VI_COUNT == len(set(abi.ENV_INERTIA_ROW_NAMES))
    assert abi.ENV_INERTIA_ROW_NAMES[abi.VI_LINK_INERTIA0 + 3] == "LINK_INERTIA[3]"
    assert abi.ENV_INERTIA_ROW_NAMES[abi.VI_AOFF1] == "AOFF[1]" and abi.ENV_INERTIA_ROW_NAMES[abi.VI_COUNT - 1] == "AOFF[4]"
    assert abi.ENV_INERTIA_NAMES == ("CART_MASS", "LINK_MASS", "TIP_LINK_MASS")
    assert not set(abi.ENV_INERTIA_NAMES) & set(abi.ENV_PARAM_NAMES) and abi.VP_COUNT == 28
    functions = sorted(set(re.findall(r"\b(vine_[a-z_0-9]+)\s*\(", text)))
    assert functions == sorted(abi.ENV_INERTIA_PROTOTYPES)
    for name in functions:
        assert hasattr(lib, name), name
    assert any(d.endswith("vine_env_inertia.h") for d in native.DEPS)


def test_row_equals_float64_numpy_field_by_field(lib, vcfg):
    vcfg.cart_mass, vcfg.gravity, vcfg.link_com = 0.73, -9.2, 0.021
    for i in range(NL):
        vcfg.link_mass[i], vcfg.link_inertia[i] = 0.004 * (i + 1.5), 3e-6 * (i + 2)
    row = env_params.inertia_config_row(lib, vcfg)
    primary = [vcfg.cart_mass] + list(vcfg.link_mass) + list(vcfg.link_inertia)
    assert np.array_equal(bits(row[:abi.VI_PRIMARY_COUNT]), bits(np.float32(primary)))
    want = expected_column(vcfg, primary)
    for r in range(abi.VI_COUNT):
        assert bits(row[r]) == bits(want[r]), (abi.ENV_INERTIA_ROW_NAMES[r], row[r], want[r])
    # every a_ij with j < i is L b_i, and g b_i carries the configuration's gravity
    L = np.float64(np.float32(vcfg.link_length))
    b = composites(np.float32(primary[0]), np.float32(primary[1:6]), np.float32(primary[6:]), np.float32(vcfg.link_length),
                   np.float32(vcfg.link_com), np.float32(vcfg.gravity))
    assert all(b[abi.VI_AOFF1 + i - 1] == L * b[abi.VI_B0 + i] for i in range(1, NL)) and row[abi.VI_GB0] < 0 < row[abi.VI_B0]
    assert lib.vine_env_inertia_row(None, (C.c_float * abi.VI_COUNT)()) == abi.ERR_INVALID_ARG


def test_derive_on_several_plants_equals_numpy_bit_for_bit(lib, vcfg):
    n = 23
    t = plants(lib, vcfg, n)
    got = env_params.derive_inertia(lib, vcfg, t)
    assert np.array_equal(bits(got[:abi.VI_PRIMARY_COUNT]), bits(t[:abi.VI_PRIMARY_COUNT]))
    for e in range(n):
        want = expected_column(vcfg, t[:abi.VI_PRIMARY_COUNT, e])
        assert np.array_equal(bits(got[:, e]), bits(want)), e
    env_params.check_inertia_table(lib, vcfg, got)
    # a column of the configuration's own float32 masses gives the configuration's own row: uniform handle = table column
    own = np.repeat(env_params.inertia_config_row(lib, vcfg)[:, None], 3, axis=1)
    again = own.copy()
    again[abi.VI_PRIMARY_COUNT:] = 0
    assert np.array_equal(bits(env_params.derive_inertia(lib, vcfg, again)), bits(own))
    assert lib.vine_env_inertia_derive(C.byref(vcfg), None, n) == abi.ERR_INVALID_ARG
    assert lib.vine_env_inertia_derive(None, got.ctypes.data, n) == abi.ERR_INVALID_ARG
    assert lib.vine_env_inertia_derive(C.byref(vcfg), got.ctypes.data, 0) == abi.ERR_INVALID_ARG


def test_check_names_each_refusal_by_row_and_env(lib, vcfg):
    n = 7
    good = env_params.derive_inertia(lib, vcfg, plants(lib, vcfg, n, seed=1))
    env_params.check_inertia_table(lib, vcfg, good)
    zero_inertia = good.copy()
    zero_inertia[abi.VI_LINK_INERTIA0 + 2, 4] = 0.0                        # a point mass is allowed
    env_params.check_inertia_table(lib, vcfg, env_params.derive_inertia(lib, vcfg, zero_inertia))
    bad = [(abi.VI_CART_MASS, 3, np.nan), (abi.VI_LINK_MASS0 + 1, 6, np.inf), (abi.VI_LINK_INERTIA0 + 4, 0, -np.inf),
           (abi.VI_GB0 + 2, 5, np.nan), (abi.VI_AOFF1 + 3, 1, np.inf),
           (abi.VI_CART_MASS, 2, 0.0), (abi.VI_CART_MASS, 0, -0.4), (abi.VI_LINK_MASS0, 1, 0.0), (abi.VI_LINK_MASS0 + 4, 6, -1e-3),
           (abi.VI_LINK_INERTIA0, 5, -1e-9), (abi.VI_LINK_INERTIA0 + 3, 2, -1.0)]
    for r, e, v in bad:
        t = good.copy()
        t[r, e] = v
        if r < abi.VI_PRIMARY_COUNT and np.isfinite(v):
            t = env_params.derive_inertia(lib, vcfg, t)                  # consistent derived rows: the primary value is the fault
        rc = lib.vine_env_inertia_check(C.byref(vcfg), t.ctypes.data, n)
        assert rc == abi.ERR_INVALID_ARG, (r, e, v)
        msg = lib.vine_last_error().decode()
        assert abi.ENV_INERTIA_ROW_NAMES[r] + " of env %d " % e in msg, msg
        with pytest.raises(ValueError, match=re.escape(abi.ENV_INERTIA_ROW_NAMES[r])):
            env_params.check_inertia_table(lib, vcfg, t)
    # every derived row, one ulp up and one ulp down, in some env
    for k, r in enumerate(range(abi.VI_PRIMARY_COUNT, abi.VI_COUNT)):
        for toward in (np.float32(np.inf), np.float32(-np.inf)):
            t, e = good.copy(), k % n
            t[r, e] = np.nextafter(t[r, e], toward)
            assert lib.vine_env_inertia_check(C.byref(vcfg), t.ctypes.data, n) == abi.ERR_INVALID_ARG, (r, toward)
            msg = lib.vine_last_error().decode()
            assert abi.ENV_INERTIA_ROW_NAMES[r] + " of env %d " % e in msg and "vine_env_inertia_derive" in msg, msg
    # a primary row changed without deriving again is caught through the rows it feeds
    stale = good.copy()
    stale[abi.VI_LINK_MASS0 + 4, 3] *= np.float32(1.25)
    assert lib.vine_env_inertia_check(C.byref(vcfg), stale.ctypes.data, n) == abi.ERR_INVALID_ARG
    assert "MTOT of env 3 " in lib.vine_last_error().decode()
    assert lib.vine_env_inertia_check(C.byref(vcfg), None, n) == abi.ERR_INVALID_ARG
    assert lib.vine_env_inertia_check(None, good.ctypes.data, n) == abi.ERR_INVALID_ARG
    assert lib.vine_env_inertia_check(C.byref(vcfg), good.ctypes.data, 0) == abi.ERR_INVALID_ARG
    with pytest.raises(ValueError, match=r"\[31, num_envs\]"):
        env_params.check_inertia_table(lib, vcfg, good[:28])


def test_null_handle(lib):
    assert lib.vine_bind_env_inertia(None, None) == abi.ERR_INVALID_ARG
    assert lib.vine_env_inertia_bound(None) == 0


# ---------------------------------------------------------------------------------------------- build_inertia_table
def test_build_inertia_table_forms_radix_and_composition(lib, vcfg):
    n = 70
    base = env_params.inertia_config_row(lib, vcfg).astype(np.float64)
    for spec in ({}, {"DAMPING": [0.01, 0.05]}, {"ACTION_DELAY": {"values": [0, 1]}, "FPAM_K": 1.1}):
        assert env_params.build_inertia_table(spec, vcfg, 3, n, lib=lib) is None
    spec = {"ACTION_DELAY": {"values": [0, 2, 5]},            # radix 3, the fastest digit
            "CART_MASS": [0.3, 0.9],
            "LINK_MASS": {"values": [0.8, 1.25]},             # the next digit
            "DAMPING": [0.01, 0.05],
            "TIP_LINK_MASS": {"values": [1.0, 1.5, 2.0, 3.0]}}            # the slowest
    t = env_params.build_inertia_table(spec, vcfg, 3, n, lib=lib)
    p = env_params.build_table(spec, vcfg, 3, n, lib=lib)
    assert t.dtype == np.float32 and t.shape == (abi.VI_COUNT, n) and p.shape == (abi.VP_COUNT, n)
    g = np.arange(n)
    assert np.array_equal(p[abi.VP_ACTION_DELAY], np.float32([0, 2, 5])[g % 3])
    link = np.float64([0.8, 1.25])[(g // 3) % 2]
    tip = np.float64([1.0, 1.5, 2.0, 3.0])[(g // 6) % 4]
    for i in range(NL):
        f = link * tip if i == NL - 1 else link               # LINK_MASS x TIP_LINK_MASS on link 4, LINK_MASS alone elsewhere
        assert np.array_equal(t[abi.VI_LINK_MASS0 + i], (base[abi.VI_LINK_MASS0 + i] * f).astype(np.float32)), i
        assert np.array_equal(t[abi.VI_LINK_INERTIA0 + i], (base[abi.VI_LINK_INERTIA0 + i] * f).astype(np.float32)), i
    # every combination of the three `values` entries, of both tables together, recurs every 3 * 2 * 4 envs
    combos = {(p[abi.VP_ACTION_DELAY, e], t[abi.VI_LINK_MASS0, e], t[abi.VI_LINK_MASS0 + 4, e] / t[abi.VI_LINK_MASS0, e]) for e in range(24)}
    assert len(combos) == 24
    assert np.array_equal(t[abi.VI_LINK_MASS0:abi.VI_PRIMARY_COUNT, :46], t[abi.VI_LINK_MASS0:abi.VI_PRIMARY_COUNT, 24:70])
    cart = t[abi.VI_CART_MASS]
    assert cart.min() >= np.float32(0.3) and cart.max() <= np.float32(0.9) and len(np.unique(cart)) > n // 2
    # the cart's draw is the stream of its own name: what build_table's hash gives for (seed, "CART_MASS", id)
    assert np.array_equal(cart, (0.3 + 0.6 * env_params.uniform01(3, "CART_MASS", g)).astype(np.float32))
    # derived rows through the library, the whole table passes its check
    assert np.array_equal(bits(t), bits(env_params.derive_inertia(lib, vcfg, t)))
    env_params.check_inertia_table(lib, vcfg, t)
    for e in (0, 17, 69):
        assert np.array_equal(bits(t[:, e]), bits(expected_column(vcfg, t[:abi.VI_PRIMARY_COUNT, e])))
    # build_table passes over the three names: its result is that of the spec without them, radix included
    without = {k: v for k, v in spec.items() if k not in abi.ENV_INERTIA_NAMES}
    q = env_params.build_table(without, vcfg, 3, n, lib=lib)
    assert np.array_equal(p, q)
    only = env_params.build_table({"CART_MASS": 0.5, "LINK_MASS": [0.9, 1.1]}, vcfg, 3, n, lib=lib)
    assert np.array_equal(only, np.repeat(env_params.config_row(lib, vcfg)[:, None], n, axis=1))
    # a number: every env; the other primary rows keep the configuration's
    s = env_params.build_inertia_table({"CART_MASS": 0.55}, vcfg, 3, n, lib=lib)
    assert np.all(s[abi.VI_CART_MASS] == np.float32(0.55))
    assert np.array_equal(s[abi.VI_LINK_MASS0:abi.VI_PRIMARY_COUNT, 5], base[abi.VI_LINK_MASS0:abi.VI_PRIMARY_COUNT].astype(np.float32))


def test_build_inertia_table_shard_is_a_slice(lib, vcfg):
    spec = {"CART_MASS": [0.3, 0.9], "LINK_MASS": [0.7, 1.4], "TIP_LINK_MASS": {"values": [1.0, 2.0, 3.0]},
            "ACTION_DELAY": {"values": [0, 1]}}
    whole = env_params.build_inertia_table(spec, vcfg, 11, 70, 0, lib=lib)
    assert np.array_equal(bits(whole), bits(env_params.build_inertia_table(spec, vcfg, 11, 70, 0, lib=lib)))
    shard = env_params.build_inertia_table(spec, vcfg, 11, 35, 35, lib=lib)
    assert np.array_equal(bits(shard), bits(whole[:, 35:70]))
    other = env_params.build_inertia_table(spec, vcfg, 12, 70, 0, lib=lib)
    assert not np.array_equal(other[abi.VI_CART_MASS], whole[abi.VI_CART_MASS])
    ratio = lambda t: np.round(t[abi.VI_LINK_MASS0 + 4].astype(np.float64) / t[abi.VI_LINK_MASS0 + 3] / 20.0, 3)   # noqa: E731
    assert np.array_equal(ratio(other), ratio(whole))                    # `values` do not draw
    # two ranged names draw from different streams
    u = (whole[abi.VI_CART_MASS] - 0.3) / 0.6
    v = (whole[abi.VI_LINK_MASS0].astype(np.float64) / np.float32(vcfg.link_mass[0]) - 0.7) / 0.7
    assert np.abs(u - v).max() > 0.3


@pytest.mark.parametrize("spec,exc,word", [
    ({"CART_MAS": 0.5}, ConfigError, "CART_MAS"),
    ({"CART_MASS": [0.9, 0.3]}, ConfigError, "CART_MASS"),
    ({"LINK_MASS": {"values": []}}, ConfigError, "LINK_MASS"),
    ({"TIP_LINK_MASS": "heavy"}, ConfigError, "TIP_LINK_MASS"),
    # both ends of a range and every listed value are checked, whatever a batch of 16 draws
    ({"CART_MASS": [0.0, 0.9]}, ValueError, "CART_MASS"),
    ({"CART_MASS": [0.3, float("inf")]}, ValueError, "CART_MASS"),
    ({"CART_MASS": {"values": [0.4, 0.5, -0.1]}}, ValueError, "CART_MASS"),
    ({"LINK_MASS": [-0.5, 1.0]}, ValueError, "LINK_MASS[0]"),
    ({"LINK_MASS": [0.5, float("nan")]}, ValueError, "LINK_MASS[0]"),
    ({"LINK_MASS": 0.0}, ValueError, "LINK_MASS[0]"),
    ({"TIP_LINK_MASS": {"values": [1.0, 2.0, 0.0]}}, ValueError, "LINK_MASS[4]"),
    ({"TIP_LINK_MASS": [-1.0, 2.0]}, ValueError, "LINK_MASS[4]"),
])
def test_build_inertia_table_refusals_name_the_row(lib, vcfg, spec, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        env_params.build_inertia_table(spec, vcfg, 1, 16, lib=lib)


def test_range_ends_are_checked_even_when_no_env_draws_them(lib, vcfg):
    """One env, whose draw lies inside (0, 0.9): the table itself would pass, the lower end 0 kg does not."""
    u = env_params.uniform01(1, "CART_MASS", [0])[0]
    assert 0.01 < u < 0.99
    with pytest.raises(ValueError, match="CART_MASS of candidate 0 "):
        env_params.build_inertia_table({"CART_MASS": [0.0, 0.9]}, vcfg, 1, 1, lib=lib)
    t = env_params.build_inertia_table({"CART_MASS": [1e-3, 0.9]}, vcfg, 1, 1, lib=lib)
    assert t[abi.VI_CART_MASS, 0] == np.float32(1e-3 + (0.9 - 1e-3) * u)


# ------------------------------------------------------------------------------------------- episodes: mass columns
def test_with_env_params_mass_columns_and_rates_by_hand(lib, vcfg):
    n = 6
    table = np.repeat(env_params.config_row(lib, vcfg)[:, None], n, axis=1)
    base = env_params.inertia_config_row(lib, vcfg)
    inertia = np.repeat(base[:, None], n, axis=1)
    inertia[abi.VI_CART_MASS] = [0.4, 0.8, 0.4, 0.8, 0.4, 0.8]
    link = np.float64([0.8, 0.8, 1.0, 1.0, 1.2, 1.2])
    for i in range(NL):
        inertia[abi.VI_LINK_MASS0 + i] = (np.float64(base[abi.VI_LINK_MASS0 + i]) * link).astype(np.float32)
    inertia = env_params.derive_inertia(lib, vcfg, inertia)
    env = np.array([0, 1, 2, 3, 4, 5, 1, 1, 3, 0], dtype=np.int64)
    reached = np.array([1, 0, 1, 1, 0, 0, 1, 0, 0, 1], dtype=np.float32)
    rows = {name: np.zeros(len(env), dtype=np.int64 if name in episodes.INT_COLUMNS else np.float32) for name in episodes.COLUMNS}
    rows["env"], rows["reached_ever"] = env, reached
    # without an inertia table: as before, no column (the parameter table is the configuration's row everywhere)
    assert not [k for k in episodes.with_env_params(rows, table, abi.ENV_PARAM_ROW_NAMES) if k.startswith("param_")]
    out = episodes.with_env_params(rows, table, abi.ENV_PARAM_ROW_NAMES, inertia)
    # one factor scales all five links: the tip's ratio to link 0 is the configuration's in every env -> no TIP column
    assert sorted(k for k in out if k.startswith("param_")) == ["param_CART_MASS", "param_LINK_MASS"]
    assert all(np.array_equal(out[k], rows[k]) for k in rows)
    assert np.array_equal(out["param_CART_MASS"], np.float32([0.4, 0.8, 0.4, 0.8, 0.4, 0.8, 0.8, 0.8, 0.8, 0.4]))
    assert np.array_equal(out["param_LINK_MASS"], inertia[abi.VI_LINK_MASS0][env])          # link 0's mass in kg
    # cart 0.4: envs 0, 2, 4, 0 -> reached 1, 1, 0, 1; cart 0.8: envs 1, 3, 5, 1, 1, 3 -> 0, 1, 0, 1, 0, 0
    values, rate, count = episodes.value_rate(out, "param_CART_MASS")
    assert values.tolist() == [float(np.float32(0.4)), float(np.float32(0.8))] and count.tolist() == [4, 6]
    assert rate.tolist() == [0.75, 2.0 / 6.0]
    # link factor 0.8: envs {0, 1} -> episodes 0, 1, 6, 7, 9 -> 1, 0, 1, 0, 1; 1.0: envs {2, 3} -> 2, 3, 8 -> 1, 1, 0; 1.2: {4, 5} -> 0, 0
    values, rate, count = episodes.value_rate(out, "param_LINK_MASS")
    assert count.tolist() == [5, 3, 2] and rate.tolist() == [0.6, 2.0 / 3.0, 0.0]
    assert np.allclose(values / np.float64(base[abi.VI_LINK_MASS0]), [0.8, 1.0, 1.2], rtol=1e-6)
    # a payload: link 4 alone scaled in two envs -> the TIP column, link 4's mass
    inertia2 = inertia.copy()
    inertia2[abi.VI_LINK_MASS0 + 4, [1, 4]] *= np.float32(2.0)
    out2 = episodes.with_env_params(rows, table, abi.ENV_PARAM_ROW_NAMES, env_params.derive_inertia(lib, vcfg, inertia2))
    assert np.array_equal(out2["param_TIP_LINK_MASS"], inertia2[abi.VI_LINK_MASS0 + 4][env])
    assert sorted(episodes.varying_params(table, abi.ENV_PARAM_ROW_NAMES, inertia2)) == ["CART_MASS", "LINK_MASS", "TIP_LINK_MASS"]


def test_npz_and_mat_hold_the_inertia_only_when_given(lib, vcfg, tmp_path):
    import scipy.io
    from vine_robot_isaacgymenvs_amd.utils import trajectory
    n = 4
    table = np.repeat(env_params.config_row(lib, vcfg)[:, None], n, axis=1)
    inertia = env_params.build_inertia_table({"CART_MASS": {"values": [0.3, 0.5, 0.7, 0.9]}}, vcfg, 0, n, lib=lib)
    rows = episodes.concat_rows([])
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    episodes.save(a, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"SUCCESS_DIST": 0.08}, table, abi.ENV_PARAM_ROW_NAMES)
    episodes.save(b, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"SUCCESS_DIST": 0.08}, table, abi.ENV_PARAM_ROW_NAMES, inertia,
                  abi.ENV_INERTIA_ROW_NAMES)
    assert episodes.load_env_inertia(a) == (None, None)
    got, names = episodes.load_env_inertia(b)
    assert np.array_equal(got, inertia) and tuple(names) == abi.ENV_INERTIA_ROW_NAMES
    assert np.array_equal(episodes.load_env_params(b)[0], table) and episodes.load(b)[3] == {"SUCCESS_DIST": 0.08}
    rec = np.zeros((3, abi.RECORD_FIELDS), dtype=np.float32)
    plain = trajectory.trajectory_arrays(rec, [0, 1, 2], 0.0333, 2, table[:, 2].astype(np.float64), abi.ENV_PARAM_ROW_NAMES)
    assert "env_inertia" not in plain
    path = trajectory.write_trajectory_mat(str(tmp_path / "t.mat"), rec, [0, 1, 2], 0.0333, 2, table[:, 2].astype(np.float64),
                                           abi.ENV_PARAM_ROW_NAMES, inertia[:, 2].astype(np.float64))
    mat = scipy.io.loadmat(path)
    assert mat["env_inertia"].shape == (abi.VI_PRIMARY_COUNT, 1)
    assert np.array_equal(mat["env_inertia"][:, 0], inertia[:abi.VI_PRIMARY_COUNT, 2].astype(np.float64))
    assert mat["env_inertia"][0, 0] == np.float64(np.float32(0.7)) and set(plain) <= set(mat)


# -------------------------------------------------------------------------------------------------- sysid: the search
def test_cem_carries_the_inertia_table_beside_the_parameter_table(lib, vcfg):
    """A synthetic error with its minimum at CART_MASS 0.6 (listed), LINK_MASS factor 1.2 (ranged) and DAMPING 0.03: the
    search gets both tables, every inertia table it evaluates passes vine_env_inertia_check, column 0 holds the best of both
    tables together from iteration 1 on, and the best error never increases."""
    from vine_robot_isaacgymenvs_amd.utils import sysid
    base, ibase = env_params.config_row(lib, vcfg), env_params.inertia_config_row(lib, vcfg)
    spec = {"CART_MASS": {"values": [0.4, 0.6, 0.8]}, "LINK_MASS": [0.7, 1.4], "DAMPING": [0.01, 0.05]}
    seen = []

    def evaluate(table, inertia):
        assert table.shape == (abi.VP_COUNT, 64) and inertia.shape == (abi.VI_COUNT, 64) and inertia.dtype == np.float32
        env_params.check_inertia_table(lib, vcfg, inertia)
        seen.append((table.copy(), inertia.copy()))
        f = inertia[abi.VI_LINK_MASS0].astype(np.float64) / np.float64(ibase[abi.VI_LINK_MASS0])
        return ((inertia[abi.VI_CART_MASS].astype(np.float64) - np.float32(0.6)) ** 2 + (f - 1.2) ** 2
                + 100.0 * (table[abi.VP_DAMPING].astype(np.float64) - 0.03) ** 2)

    inertia = (ibase, lambda t: env_params.derive_inertia(lib, vcfg, t), lambda t: env_params.check_inertia_table(lib, vcfg, t))
    best, err, history = sysid.cem(evaluate, spec, base, 64, 6, seed=5, check=lambda t: env_params.check_table(lib, vcfg, t),
                                   inertia=inertia)
    ibest = history[-1]["inertia_best"]
    assert best.shape == (abi.VP_COUNT,) and ibest.shape == (abi.VI_COUNT,) and history[-1]["inertia"].shape == (abi.VI_COUNT, 64)
    assert ibest[abi.VI_CART_MASS] == np.float32(0.6)
    assert abs(ibest[abi.VI_LINK_MASS0] / ibase[abi.VI_LINK_MASS0] - 1.2) < 0.02 and abs(best[abi.VP_DAMPING] - 0.03) < 2e-3
    assert err < 1e-3 and [h["best_error"] for h in history] == sorted([h["best_error"] for h in history], reverse=True)
    # iteration 0 is the builders' own draw; later column 0 is the best so far of both tables
    assert np.array_equal(seen[0][1], env_params.build_inertia_table(spec, vcfg, 5, 64, lib=lib))
    assert np.array_equal(seen[0][0], env_params.build_table(spec, vcfg, 5, 64, lib=lib))
    for it in range(1, 6):
        prev_t, prev_i = seen[it - 1]
        e = evaluate(prev_t, prev_i); seen.pop()
        k = int(np.argmin(e))
        if e[k] <= history[it - 1]["best_error"]:
            assert np.array_equal(seen[it][0][:, 0], prev_t[:, k]) and np.array_equal(bits(seen[it][1][:, 0]), bits(prev_i[:, k]))
    assert set(history[0]["counts"]) == {"CART_MASS"} and set(history[0]["ranges"]) == {"LINK_MASS", "DAMPING"}
    lo, hi = history[-1]["ranges"]["LINK_MASS"]
    assert 0.7 <= lo < 1.2 < hi <= 1.4 and hi - lo < 0.35
    with pytest.raises(ValueError, match="needs inertia"):
        sysid.cem(lambda t: np.zeros(8), {"CART_MASS": [0.3, 0.9]}, base, 8, 1, seed=0, check=lambda t: t)
    # a spec without the three names: evaluate keeps its one argument, no inertia keys
    _, _, h = sysid.cem(lambda t: (t[abi.VP_DAMPING] - 0.03) ** 2, {"DAMPING": [0.01, 0.05]}, base, 16, 2, seed=0,
                        check=lambda t: env_params.check_table(lib, vcfg, t))
    assert "inertia" not in h[-1] and "inertia_best" not in h[-1]


# ------------------------------------------------------------------------ the nine mass sets of the GPU tests, on the oracle
def test_oracle_is_finite_and_within_tolerance_on_every_mass_set(lib):
    """tests/env_inertia_sets.py: on each of the nine sets the oracle's float32 build stays finite and within the tolerances
    the GPU tests hold the kernel to against its float64 build -- one step from a random mid-episode state at
    single_step_case's float64 tolerances, then 40 steps at test_trajectory_tracks_oracle's -- the tolerances and the
    procedure of test_env_params_cpu.py for its nine sets, so a miss on the GPU is the kernel's, not the sets'.  Cart mass and
    every link mass and inertia differ between any two sets."""
    from oracle import vine_oracle as vo
    from tests.env_inertia_sets import HI, LO, NUM_SETS, set_cfg, set_rows
    from tests.helpers import base_cfg, random_state
    from tests.test_hip_parity import QPOS, compare_step
    n, T = 70, 40
    cfg0 = base_cfg(n, randomize=True, max_episode_length=12, seed=77)
    rows = set_rows(lib, cfg0)
    own = env_params.inertia_config_row(lib, cfg0)
    for a in range(NUM_SETS):
        for b in range(a + 1, NUM_SETS):
            assert np.all(rows[a, :abi.VI_PRIMARY_COUNT] != rows[b, :abi.VI_PRIMARY_COUNT]), (a, b)
            assert np.all(rows[a, abi.VI_PRIMARY_COUNT:] != rows[b, abi.VI_PRIMARY_COUNT:]), (a, b)
    fac = rows[:, :abi.VI_PRIMARY_COUNT].astype(np.float64) / own[:abi.VI_PRIMARY_COUNT]
    assert fac.min() > LO - 1e-6 and fac.max() < HI + 1e-6 and np.ptp(fac, axis=0).min() > 0.59
    env_params.check_inertia_table(lib, cfg0, np.ascontiguousarray(rows.T))
    for g in range(NUM_SETS):
        cfg = set_cfg(cfg0, g)
        cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
        rng = np.random.default_rng(100 + g)
        lo, hi = vo.OracleEnv(cfg, "f32"), vo.OracleEnv(cfg, "f64")
        st = random_state(rng, n, cfg)
        reset = (rng.uniform(size=n) < 0.15).astype(np.int64)
        progress = rng.integers(0, cfg.max_episode_length - 1, n)
        progress[: n // 16] = cfg.max_episode_length - 2
        for o in (lo, hi):
            o.state[:] = st.astype(o.real)
            o.reset_buf[:], o.progress[:], o.step_count = reset, progress, 7
        actions = rng.uniform(-1.3, 1.3, (n, 2))
        lo.step(actions); hi.step(actions)
        assert np.isfinite(lo.state).all() and np.isfinite(lo.obs).all()
        compare_step((lo.obs, lo.rew, lo.reset_buf, lo.timeouts), hi, lo, 1e-4, 1e-2, 1e-2)
        lo.close(); hi.close()
        cfg = set_cfg(cfg0, g)
        lo, hi = vo.OracleEnv(cfg, "f32"), vo.OracleEnv(cfg, "f64")
        mismatched, worst_q = np.zeros(n, bool), 0.0
        for t in range(T):
            a = rng.uniform(-1, 1, (n, 2))
            lo.step(a); hi.step(a)
            mismatched |= lo.reset_buf != hi.reset_buf
            ok = ~mismatched
            assert np.isfinite(lo.state).all()
            worst_q = max(worst_q, np.abs(lo.state[QPOS][:, ok].astype(np.float64) - hi.state[QPOS][:, ok]).max())
            np.testing.assert_allclose(lo.obs[ok], hi.obs[ok], rtol=0, atol=2e-2)
            np.testing.assert_allclose(lo.rew[ok], hi.rew[ok], rtol=1e-4, atol=5e-3)
            np.testing.assert_array_equal(lo.progress[ok], hi.progress[ok])
        print("mass set %d: mismatched %d of %d, worst |dq| %.3g" % (g, mismatched.sum(), n, worst_q))
        assert mismatched.mean() < 0.02 and worst_q < 5e-3
        lo.close(); hi.close()
