"""The named draw (utils/named_draw.py) without a GPU: every draw and every packing of the seven functions that existed
before there was one module, recorded then (tests/golden/named_draw_parent.npz holds its own inputs), against what those names
give now, bit for bit; that all of them reach the one loop; that no module under utils/ borrows another's private name; and
the shared host check of csrc/vine_named_draw.h through two spec entry points, as a stand-alone program under the host's
sanitizers."""
import ast
import json
import os
import subprocess

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, env_push, env_sensor, env_target, mpc_filter, mpc_observe, named_draw

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = {"env_params": env_params, "env_sensor": env_sensor, "env_push": env_push, "env_target": env_target,
           "mpc_observe": mpc_observe, "mpc_filter": mpc_filter}


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(REPO, "tests", "golden", "named_draw_parent.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(str(arrays.pop("cases")[()])), arrays


def bits(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x.view(np.uint64)


def drawn_now(case):
    """What the function a case names gives today for the case's own inputs, as float64 [S, M]."""
    module, function = case["func"].split(".")
    spec, seed, ids, episodes = case["spec"], int(case["seed"]), np.asarray(case["ids"], dtype=np.int64), case["episodes"]
    if module == "env_params":            # (``_draw`` was ``_draw_episode`` at episode 0 by construction: it is no more)
        d = env_params._draw_episode(env_params.spec_forms(spec), seed, ids, 0 if function == "_draw" else episodes)
        return np.stack([d[name] for name in spec])
    fn = getattr(MODULES[module], function)
    return fn(spec, seed, ids) if episodes is None else fn(spec, seed, ids, episodes)


def test_every_recorded_draw_bit_for_bit(recorded):
    cases, arrays = recorded
    seen = set()
    for case in cases["draws"]:
        want = arrays[case["out"]]
        got = drawn_now(case)
        assert got.dtype == np.float64 and got.shape == want.shape, case["func"]
        assert np.array_equal(bits(got), bits(want)), (case["func"], case["seed"], case["spec"])
        seen.add(case["func"])
        assert set(case["ids"]) == {0, 1, 2, 3, 5, 69, 1000, 2 ** 31 + 5} and int(case["seed"]) in (0, 2 ** 63 + 11)
        assert case["episodes"] is None or set(case["episodes"]) == {0, 1, 2, 7}
    assert seen == {"env_params._draw", "env_params._draw_episode", "env_sensor.draw_sensor", "env_push.draw_push",
                    "env_target.draw_target", "mpc_observe.draw_observe", "mpc_filter.draw_gains"}
    assert not hasattr(env_params, "_draw")


def test_every_recorded_packing_byte_for_byte(recorded):
    cases, arrays = recorded
    seen = set()
    for case in cases["packs"]:
        module, function = case["func"].split(".")
        names, values = getattr(MODULES[module], function)(case["spec"])
        assert np.array_equal(np.frombuffer(bytes(names), dtype=np.uint8), arrays[case["names"]]), case["func"]
        assert values.dtype == np.float64 and np.array_equal(bits(values), bits(arrays[case["values"]])), case["func"]
        seen.add(case["func"])
    assert seen == {"env_params.redraw_names", "env_sensor.sensor_names", "env_push.push_names", "env_target.target_names"}
    names, _ = env_params.redraw_names({"ACTION_DELAY": [0, 3]})          # a name nobody fills stays ABSENT, in its slot
    forms = [nm.form for nm in names]
    assert len(names) == abi.VR_NAMES and forms[abi.ENV_REDRAW_NAMES.index("ACTION_DELAY")] == abi.REDRAW_RANGE
    assert forms.count(abi.REDRAW_ABSENT) == abi.VR_NAMES - 1


def test_every_draw_reaches_the_one_loop(monkeypatch):
    sensor = {"DELAY": [0, 3], "HOLD": 0.1, "NOISE_STD": {"values": [0.0, 0.01]}}
    push = {"RATE": [0.0, 1.0], "IMPULSE": 0.1}
    target = {"VEL_ALONG": [-0.1, 0.1], "VEL_ACROSS": 0.0, "SPAN_ALONG": 0.1, "SPAN_ACROSS": 0.0}
    observe = {"DELAY": [0, 2], "HOLD": 0.0, "NOISE_Q": 0.0, "NOISE_QD": 0.0}
    gains = {"GAIN_Q": [0.1, 0.2], "GAIN_QD": 0.3}
    calls = [lambda: env_sensor.draw_sensor(sensor, 1, [0, 1], [0, 1]), lambda: env_push.draw_push(push, 1, [0, 1], [0, 1]),
             lambda: env_target.draw_target(target, 1, [0, 1], [0, 1]), lambda: mpc_observe.draw_observe(observe, 1, [0, 1]),
             lambda: mpc_filter.draw_gains(gains, 1, [0, 1]),
             lambda: env_params._draw_episode(env_params.spec_forms({"DAMPING": [0.1, 0.2]}), 1, [0, 1], [0, 1]),
             lambda: env_params.draw_table({"DAMPING": [0.1, 0.2]}, np.ones(abi.VP_COUNT, dtype=np.float32), 1, 2)]
    before = [c() for c in calls]
    real, counted = named_draw.draw, []

    def shifted(named_forms, *args, **kwargs):
        counted.append([name for name, _ in named_forms])
        return real(named_forms, *args, **kwargs) + 1.0

    monkeypatch.setattr(named_draw, "draw", shifted)
    after = [c() for c in calls]
    assert len(counted) == len(calls)
    for a, b in zip(before[:-1], after[:-1]):
        a, b = (np.stack(list(x.values())) if isinstance(x, dict) else x for x in (a, b))
        assert np.array_equal(b, a + 1.0)
    assert np.array_equal(after[-1][abi.VP_DAMPING], (before[-1][abi.VP_DAMPING].astype(np.float64) + 1.0).astype(np.float32))
    assert counted[0] == list(env_sensor.DRAW_NAMES) and counted[3] == list(mpc_observe.DRAW_NAMES)
    # the hash, the parser and the packing have one statement too
    assert env_params.uniform01_episode is named_draw.uniform01_episode and env_params.name_key is named_draw.name_key
    assert env_sensor.philox4x32_10 is named_draw.philox4x32_10 is env_push.philox4x32_10
    source = {name: open(m.__file__).read() for name, m in MODULES.items()}
    for name, text in source.items():
        assert "isinstance(form, dict)" not in text and "radix *=" not in text and "radix =" not in text, name
        assert "def _form" not in text and "def _candidates" not in text.replace("def _candidates(forms)", ""), name


def test_no_module_under_utils_imports_an_underscore_name_of_another():
    utils = os.path.join(REPO, "vine_robot_isaacgymenvs_amd", "utils")
    modules = sorted(f[:-3] for f in os.listdir(utils) if f.endswith(".py") and f != "__init__.py")
    assert "named_draw" in modules
    for module in modules:
        tree = ast.parse(open(os.path.join(utils, module + ".py")).read())
        aliases = {}                      # local name -> module of utils/ it stands for
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level >= 1:
                for a in node.names:
                    if node.level == 1 and node.module is None and a.name in modules:
                        aliases[a.asname or a.name] = a.name
                    elif node.module is not None:
                        assert not a.name.startswith("_"), "%s imports %s from %s" % (module, a.name, node.module)
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in aliases:
                if aliases[node.value.id] != module:
                    assert not (node.attr.startswith("_") and not node.attr.startswith("__")), \
                        "%s uses %s.%s" % (module, node.value.id, node.attr)


def test_the_shared_refusals_through_the_stand_alone_host_check(tmp_path):
    """scripts/named_draw_host_check.cpp, built as its head says -- the HOST code of the push's and the sensor's units under
    AddressSanitizer and UBSan -- walks the eight refusals of ``named_check`` through ``vine_env_push_spec`` and
    ``vine_env_sensor_spec``.  A few seconds of hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "named_draw_host_check")
    source = os.path.join(REPO, "scripts", "named_draw_host_check.cpp")
    text = open(source).read()
    header = open(os.path.join(os.path.dirname(native.SRC_PUSH), "vine_named_draw.h")).read()
    for word in ("reserved must be 0", "the number is not finite", "a range needs finite lo <= hi",
                 "the extent of the value list lies outside the values array", "radix must be at least 1",
                 "a listed value is not finite", "absent: every name needs a number, a range or a value list", "unknown form"):
        assert word in text and header.count('"%s"' % word) == 1, word
        for unit in (native.SRC_PUSH, native.SRC_SENSOR, native.SRC_TARGET, native.SRC_REDRAW):
            assert word not in open(unit).read(), (word, unit)
    subprocess.check_call([hipcc, "--offload-arch=" + native.ARCH, "-O1", "-g", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-x", "hip",
                           source, native.SRC_PUSH, native.SRC_SENSOR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "named draw host check ok" in out.stdout, out.stdout + out.stderr
