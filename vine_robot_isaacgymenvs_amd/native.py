"""Build and load ``libvine_hip.so`` — the only compute backend of this package.

There is deliberately no CPU fallback: if the HIP extension is missing or no MI355X is
visible, loading/creating fails loudly.
"""
import ctypes as C
import hashlib
import os
import subprocess

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "vine_hip.hip")
SRC_PPO = os.path.join(_HERE, "csrc", "ppo_kernels.hip")
SRC_RENDER = os.path.join(_HERE, "csrc", "vine_render.hip")
SRC_RECORD = os.path.join(_HERE, "csrc", "vine_record.hip")
SRC_EPISODES = os.path.join(_HERE, "csrc", "vine_episodes.hip")
SRC_SYSID = os.path.join(_HERE, "csrc", "vine_sysid.hip")
SRC_REDRAW = os.path.join(_HERE, "csrc", "vine_env_redraw.hip")
SRC_ADR = os.path.join(_HERE, "csrc", "vine_env_adr.hip")
SRC_SENSOR = os.path.join(_HERE, "csrc", "vine_env_sensor.hip")
SOURCES = (SRC, SRC_PPO, SRC_RENDER, SRC_RECORD, SRC_EPISODES, SRC_SYSID, SRC_REDRAW, SRC_ADR)
# tests/test_env_params_adr_cpu.py pins SOURCES to the eight units above, in this order; the ninth, the sensor's, follows them
# in UNITS, which is what build() compiles and links
UNITS = SOURCES + (SRC_SENSOR,)
# tests/test_env_sensor_cpu.py pins UNITS to those nine in turn; the tenth, the push's, follows them in BUILD_UNITS, which is
# what build() compiles and links
SRC_PUSH = os.path.join(_HERE, "csrc", "vine_env_push.hip")
BUILD_UNITS = UNITS + (SRC_PUSH,)
# tests/test_env_push_cpu.py pins BUILD_UNITS to those ten in turn; the eleventh, the predictive controller's, follows them in
# ALL_UNITS, which is what build() compiles and links
SRC_MPC = os.path.join(_HERE, "csrc", "vine_mpc.hip")
ALL_UNITS = BUILD_UNITS + (SRC_MPC,)
# tests/test_mpc_cpu.py pins ALL_UNITS to those eleven in turn; the twelfth, the controller's model adaptation, follows them in
# LIB_UNITS, which is what build() compiles and links
SRC_MPC_ADAPT = os.path.join(_HERE, "csrc", "vine_mpc_adapt.hip")
LIB_UNITS = ALL_UNITS + (SRC_MPC_ADAPT,)
# tests/test_mpc_adapt_cpu.py pins LIB_UNITS to those twelve in turn; the thirteenth, the controller's policy proposal, follows
# them in POLICY_UNITS, which is what build() compiles and links
SRC_MPC_POLICY = os.path.join(_HERE, "csrc", "vine_mpc_policy.hip")
POLICY_UNITS = LIB_UNITS + (SRC_MPC_POLICY,)
# tests/test_mpc_policy_cpu.py pins POLICY_UNITS to those thirteen in turn, and the loop of build() over them; the fourteenth, the
# controller's sensing path, follows them there: build() compiles and links POLICY_UNITS + (SRC_MPC_OBSERVE,)
SRC_MPC_OBSERVE = os.path.join(_HERE, "csrc", "vine_mpc_observe.hip")
# tests/test_mpc_observe_cpu.py pins that spelling of the loop; the fifteenth, the corrector over the sensing path's frames,
# follows it there: build() compiles and links POLICY_UNITS + (SRC_MPC_OBSERVE,) + (SRC_MPC_FILTER,)
SRC_MPC_FILTER = os.path.join(_HERE, "csrc", "vine_mpc_filter.hip")
# tests/test_mpc_filter_cpu.py pins that spelling in turn; the sixteenth, the moving target's, follows it there: build() compiles
# and links POLICY_UNITS + (SRC_MPC_OBSERVE,) + (SRC_MPC_FILTER,) + (SRC_TARGET,)
SRC_TARGET = os.path.join(_HERE, "csrc", "vine_env_target.hip")
# tests/test_env_target_cpu.py pins that spelling, colon included; the seventeenth, the controller's target tracking, cannot join
# the expression: build() hands it to the loop's body (a local helper) once more behind the loop
SRC_MPC_TRACK = os.path.join(_HERE, "csrc", "vine_mpc_track.hip")
# tests/test_mpc_track_cpu.py pins that call and the number of calls build() spells out; the eighteenth, the ADR of the sensor's,
# the push's and the target's draws, follows in LATER_UNITS, which build() maps the same helper over
SRC_DRAW_ADR = os.path.join(_HERE, "csrc", "vine_env_draw_adr.hip")
LATER_UNITS = (SRC_DRAW_ADR,)
# tests/test_env_draw_adr_cpu.py pins LATER_UNITS to that one and the line of build() that maps the helper over it; the
# nineteenth, the controller's sample distribution, follows in NOISE_UNITS, which build() maps the same helper over behind it
SRC_MPC_NOISE = os.path.join(_HERE, "csrc", "vine_mpc_noise.hip")
NOISE_UNITS = (SRC_MPC_NOISE,)
# tests/test_mpc_noise_cpu.py pins NOISE_UNITS to that one and the line of build() that maps the helper over it; the twentieth,
# the mass dimensions of the controller's model adaptation, follows in INERTIA_UNITS, which build() maps the helper over behind it
SRC_MPC_ADAPT_INERTIA = os.path.join(_HERE, "csrc", "vine_mpc_adapt_inertia.hip")
INERTIA_UNITS = (SRC_MPC_ADAPT_INERTIA,)
# tests/test_mpc_adapt_inertia_cpu.py pins INERTIA_UNITS to that one and the line of build() that maps the helper over it; the
# twenty-first, the controller's ensemble of candidate plants, follows in ENSEMBLE_UNITS, which build() maps the helper over behind it
SRC_MPC_ENSEMBLE = os.path.join(_HERE, "csrc", "vine_mpc_ensemble.hip")
ENSEMBLE_UNITS = (SRC_MPC_ENSEMBLE,)
LIB = os.path.join(_HERE, "libvine_hip.so")
ARCH = "gfx950"

FINGERPRINT = LIB + ".fingerprint"
_INC = os.path.join(os.path.dirname(_HERE), "include")
_HEADERS = ([os.path.join(_INC, h) for h in ("vine.h", "vine_ppo.h", "vine_render.h", "vine_record.h", "vine_episodes.h",
                                              "vine_env_params.h", "vine_env_inertia.h", "vine_sysid.h")]
            + [os.path.join(_HERE, "csrc", h) for h in ("vine_task_shared.h", "vine_geometry.h", "vine_observer.h",
                                                        "vine_policy_head.h", "vine_ppo_formulas.h")])
# what only some translation units include and compile with: the others' objects do not depend on it
_COMPOSITES = os.path.join(_HERE, "csrc", "vine_inertia_composites.h")
# the named draw (csrc/vine_named_draw.h): what the sensor, the push and the target include of it; the redraw and ADR also
# form table columns (csrc/vine_env_redraw_draw.h, which needs the composites)
_NAMED_DRAW_HEADERS = [os.path.join(_INC, "vine_env_redraw.h"), os.path.join(_HERE, "csrc", "vine_named_draw.h")]
_REDRAW_HEADERS = [_COMPOSITES] + _NAMED_DRAW_HEADERS + [os.path.join(_HERE, "csrc", "vine_env_redraw_draw.h")]
_MPC_SHARED = os.path.join(_HERE, "csrc", "vine_mpc_shared.h")      # the fork's and the pin's column copy and ring rebuild
_TARGET_PATH = os.path.join(_HERE, "csrc", "vine_target_path.h")    # the target's path step and the words of a point of it
_ADR_SHARED = os.path.join(_HERE, "csrc", "vine_adr_shared.h")      # a boundary after w steps and the decide launch's lane
_SOURCE_HEADERS = {SRC: [_COMPOSITES], SRC_REDRAW: _REDRAW_HEADERS, SRC_ADR: _REDRAW_HEADERS + [os.path.join(_INC, "vine_env_adr.h"), _ADR_SHARED],
                   SRC_DRAW_ADR: _NAMED_DRAW_HEADERS + [os.path.join(_INC, h) for h in ("vine_env_adr.h", "vine_env_sensor.h",
                                                                                         "vine_env_push.h", "vine_env_target.h",
                                                                                         "vine_env_draw_adr.h")] + [_ADR_SHARED],
                   SRC_SENSOR: _NAMED_DRAW_HEADERS + [os.path.join(_INC, "vine_env_sensor.h")],
                   SRC_PUSH: _NAMED_DRAW_HEADERS + [os.path.join(_INC, "vine_env_push.h")],
                   SRC_TARGET: _NAMED_DRAW_HEADERS + [os.path.join(_INC, "vine_env_target.h"), _TARGET_PATH],
                   SRC_MPC_TRACK: [os.path.join(_INC, "vine_env_redraw.h"), os.path.join(_INC, "vine_env_target.h"),
                                   os.path.join(_INC, "vine_mpc.h"), os.path.join(_INC, "vine_mpc_track.h"), _TARGET_PATH],
                   SRC_MPC: [os.path.join(_INC, "vine_mpc.h"), _MPC_SHARED],
                   SRC_MPC_NOISE: [os.path.join(_INC, "vine_mpc.h"), os.path.join(_INC, "vine_mpc_noise.h"), _MPC_SHARED],
                   SRC_MPC_ENSEMBLE: [os.path.join(_INC, "vine_mpc.h"), os.path.join(_INC, "vine_mpc_ensemble.h"), _MPC_SHARED],
                   SRC_MPC_ADAPT: [os.path.join(_INC, "vine_mpc.h"), os.path.join(_INC, "vine_mpc_adapt.h"), _MPC_SHARED],
                   SRC_MPC_ADAPT_INERTIA: [os.path.join(_INC, "vine_mpc.h"), os.path.join(_INC, "vine_mpc_adapt.h"),
                                           os.path.join(_INC, "vine_mpc_adapt_inertia.h"), _COMPOSITES, _MPC_SHARED],
                   SRC_MPC_POLICY: [os.path.join(_INC, "vine_mpc.h"), os.path.join(_INC, "vine_mpc_policy.h"), _MPC_SHARED],
                   SRC_MPC_OBSERVE: [os.path.join(_INC, "vine_mpc_observe.h"), _MPC_SHARED],
                   SRC_MPC_FILTER: [os.path.join(_INC, "vine_mpc_observe.h"), os.path.join(_INC, "vine_mpc_filter.h"), _MPC_SHARED]}
# vine_env_redraw.hip forms table columns that must hold the bits numpy and the host pass give: a + b * c stays a multiply
# and an add (under -ffp-contract=fast hipcc fuses it on gfx950, a pragma in the source notwithstanding)
# vine_env_adr.hip forms the same columns and the range in force: it switches contraction off itself, by a pragma in front of
# everything it includes, which this spelling of the flag makes the compiler honour (plain "fast" ignores the pragma)
# vine_env_sensor.hip adds noise to an observation, obs + z * c, that numpy must reproduce bit for bit: the pragma and the flag
# of vine_env_adr.hip
# vine_env_push.hip draws its two per-env values with the same statement, and its solve is the float32 statement numpy makes:
# the same pragma and flag
# vine_mpc.hip forms a sample's action, nominal + z * c, that numpy must reproduce bit for bit: the same pragma and flag
# vine_mpc_adapt.hip forms a candidate's value, mean + z * std, and the belief's update in float64 the same way: the same again
# vine_mpc_policy.hip forms an action, mu + d, and a cost, cost - w * V, that numpy must reproduce bit for bit: the same again
# vine_mpc_observe.hip forms a measured joint value, q + z * c, that numpy must reproduce bit for bit: the same again
# vine_mpc_filter.hip forms a corrected joint value, x + g * (y - x), that numpy must reproduce bit for bit: the same again
# vine_env_target.hip forms an offset, off + vel * cdt, a target, ay - off * c, and an observation column, obs + w * inv, that
# numpy must reproduce bit for bit: the same again
# vine_mpc_track.hip forms the same offsets and targets H - 1 steps ahead, bit for bit those of vine_env_target.hip: the same again
# vine_env_draw_adr.hip forms the range in force and draws from it as vine_env_adr.hip does: the same again
# vine_mpc_noise.hip forms a perturbation, b * eps + g * z, and vine_mpc.hip's action around it, bit for bit numpy's: the same again
# vine_mpc_adapt_inertia.hip forms a candidate mass, mean + z * std, and the composites of a column, m l + L distal, bit for bit
# those of numpy and of vine_env_inertia_derive: the same again
# vine_mpc_ensemble.hip forms vine_mpc.hip's action for a group and a group's cost, cmax + log(sum / E) / theta, in the float64
# operations numpy performs: the same again
_SOURCE_FLAGS = {SRC_REDRAW: ["-ffp-contract=off"], SRC_ADR: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_SENSOR: ["-ffp-contract=fast-honor-pragmas"], SRC_PUSH: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC: ["-ffp-contract=fast-honor-pragmas"], SRC_MPC_ADAPT: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC_POLICY: ["-ffp-contract=fast-honor-pragmas"], SRC_MPC_OBSERVE: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC_FILTER: ["-ffp-contract=fast-honor-pragmas"], SRC_TARGET: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC_TRACK: ["-ffp-contract=fast-honor-pragmas"], SRC_DRAW_ADR: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC_NOISE: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC_ADAPT_INERTIA: ["-ffp-contract=fast-honor-pragmas"],
                 SRC_MPC_ENSEMBLE: ["-ffp-contract=fast-honor-pragmas"]}
DEPS = (list(UNITS) + _HEADERS + _SOURCE_HEADERS[SRC_ADR] + [os.path.join(_INC, "vine_env_sensor.h")]
        + [SRC_PUSH, os.path.join(_INC, "vine_env_push.h")] + [SRC_MPC, os.path.join(_INC, "vine_mpc.h")]
        + [SRC_MPC_ADAPT, os.path.join(_INC, "vine_mpc_adapt.h"), _MPC_SHARED]
        + [SRC_MPC_POLICY, os.path.join(_INC, "vine_mpc_policy.h")]
        + [SRC_MPC_OBSERVE, os.path.join(_INC, "vine_mpc_observe.h")]
        + [SRC_MPC_FILTER, os.path.join(_INC, "vine_mpc_filter.h")]
        + [SRC_TARGET, os.path.join(_INC, "vine_env_target.h")]
        + [SRC_MPC_TRACK, os.path.join(_INC, "vine_mpc_track.h"), _TARGET_PATH]
        + [SRC_DRAW_ADR, os.path.join(_INC, "vine_env_draw_adr.h"), _ADR_SHARED]
        + [SRC_MPC_NOISE, os.path.join(_INC, "vine_mpc_noise.h")]
        + [SRC_MPC_ADAPT_INERTIA, os.path.join(_INC, "vine_mpc_adapt_inertia.h")]
        + [SRC_MPC_ENSEMBLE, os.path.join(_INC, "vine_mpc_ensemble.h")])

_lib = None


def source_fingerprint():
    """sha256 over the kernel sources and the headers: what a built library must correspond to."""
    h = hashlib.sha256()
    for d in DEPS:
        with open(d, "rb") as f:
            h.update(f.read())
    h.update(os.environ.get("VINE_HIPCC_FLAGS", "").encode())
    return h.hexdigest()


def is_fresh():
    try:
        return os.path.exists(LIB) and open(FINGERPRINT).read().strip() == source_fingerprint()
    except OSError:
        return False


def _flags(src=None):
    flags = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-fno-slp-vectorize", "-Wall",
             "-Wno-unused-function"] + _SOURCE_FLAGS.get(src, [])      # (a later -ffp-contract wins)
    extra = os.environ.get("VINE_HIPCC_FLAGS")       # experiments only (e.g. "-fslp-vectorize"); after the defaults, so they win
    return flags + (extra.split() if extra else [])


def _object_fingerprint(src):
    h = hashlib.sha256()
    for d in [src] + _HEADERS + _SOURCE_HEADERS.get(src, []):
        with open(d, "rb") as f:
            h.update(f.read())
    h.update(" ".join(_flags(src)).encode())
    return h.hexdigest()


def build(force=False, verbose=False):
    """hipcc cross-compiles for gfx950 (works without a GPU); output stays in-tree.  The seventeen translation units and the
    eighteenth to twenty-first behind them (``LATER_UNITS``, ``NOISE_UNITS``, ``INERTIA_UNITS``, ``ENSEMBLE_UNITS``) are compiled side by side into ``build/obj`` (each object is reused while its source, the headers and the flags are
    unchanged) and linked into the one library.  A sidecar fingerprint of the sources is written next to the library:
    ``load()`` refuses to call into a library built from other sources (a stale binary behind a changed C signature is a
    wild pointer on the GPU)."""
    if not force and is_fresh():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(os.path.dirname(_HERE), "build", "obj")
    os.makedirs(objdir, exist_ok=True)
    if os.path.exists(FINGERPRINT):
        os.remove(FINGERPRINT)
    jobs, objs = [], []

    def compile_unit(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        fp = _object_fingerprint(src)
        try:
            fresh = not force and os.path.exists(obj) and open(obj + ".fingerprint").read().strip() == fp
        except OSError:
            fresh = False
        if fresh:
            return
        cmd = [hipcc] + _flags(src) + ["-c", "-o", obj, src]
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        if os.path.exists(obj + ".fingerprint"):
            os.remove(obj + ".fingerprint")
        jobs.append((subprocess.Popen(cmd), cmd, obj, fp))

    for src in POLICY_UNITS + (SRC_MPC_OBSERVE,) + (SRC_MPC_FILTER,) + (SRC_TARGET,):
        compile_unit(src)
    compile_unit(SRC_MPC_TRACK)      # the seventeenth: started before any of the sixteen is waited for
    for _ in map(compile_unit, LATER_UNITS):      # the eighteenth: likewise
        pass
    for _ in map(compile_unit, NOISE_UNITS):      # the nineteenth: likewise
        pass
    for _ in map(compile_unit, INERTIA_UNITS):      # the twentieth: likewise
        pass
    for _ in map(compile_unit, ENSEMBLE_UNITS):      # the twenty-first: likewise
        pass
    for proc, cmd, obj, fp in jobs:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
        with open(obj + ".fingerprint", "w") as f:
            f.write(fp + "\n")
    subprocess.check_call([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs)
    with open(FINGERPRINT, "w") as f:
        f.write(source_fingerprint() + "\n")
    return LIB


def load():
    """Return the ctypes handle of libvine_hip.so with prototypes attached."""
    global _lib
    if _lib is None and os.environ.get("VINE_HIP_LIB"):
        # experiments only (A/B builds of the kernels with other compile flags): load exactly this file
        import torch  # noqa: F401
        _lib = abi.declare_all(C.CDLL(os.environ["VINE_HIP_LIB"]))
        return _lib
    if _lib is None:
        # PyTorch-ROCm ships its own libamdhip64.so.7; it must be the HIP runtime of the process, so it is
        # loaded first (two runtimes in one process do not both see the device).
        import torch  # noqa: F401
        if not os.path.exists(LIB):
            raise RuntimeError(
                "libvine_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or vine_robot_isaacgymenvs_amd.native.build(); this package has no CPU fallback." % LIB)
        if not is_fresh():
            # sources changed since the build (or the sidecar is missing): rebuild in place when a compiler is
            # here, otherwise stop -- never run a binary whose ABI may not match abi.py
            if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
                import fcntl
                with open(LIB + ".lock", "w") as lock:      # ranks of one job: one of them rebuilds, the others wait
                    fcntl.flock(lock, fcntl.LOCK_EX)
                    if not is_fresh():
                        print("libvine_hip.so does not match the sources: rebuilding (hipcc, ~2 min)", flush=True)
                        build()
            else:
                raise RuntimeError("libvine_hip.so was built from different sources and no hipcc is available")
        _lib = abi.declare_all(C.CDLL(LIB))
    return _lib


def check(rc, lib=None):
    if rc == abi.OK:
        return
    lib = lib or load()
    msg = lib.vine_last_error().decode(errors="replace")
    if rc == abi.ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == abi.ERR_INVALID_ARG:
        raise ValueError(msg)
    raise RuntimeError("libvine_hip error %d: %s" % (rc, msg))
