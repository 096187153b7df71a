"""What the MPC controllers and ``mpc.play`` state once, without a GPU: the table of refused combinations against the
messages the code raised before there was a table, and the run loop of ``mpc.Controller`` -- units replayed from a boundary,
eager steps elsewhere -- on stubs that count what a device would do."""
import pytest

from vine_robot_isaacgymenvs_amd.learning import graph_capture
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_adapt
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

# ---- the rule table.  The keys and messages below were recorded from play() as it stood before the table (the commit
# "ENV_DRAW_ADR: sensor, push and target ranges widen on device as mastered"), called with exactly these keys.
RECORDED = (
    (("track", "!ENV_TARGET"), "mpc: track= needs a plant with task.env.ENV_TARGET: there is no path to follow"),
    (("track", "policy"), "mpc: track= together with policy= is refused: the samples' observation would need the target's "
                          "velocity columns"),
    (("track", "adapt"), "mpc: track= together with adapt= is refused: the adaptive controller's traces were built for a "
                         "resting target"),
    (("track", "observe"), "mpc: track= together with observe= or filter= is refused: the predictor was built for a resting "
                           "target"),
    (("track", "filter"), "mpc: track= together with observe= or filter= is refused: the predictor was built for a resting "
                          "target"),
    (("filter", "!observe"), "mpc: filter= needs observe=: the frames it corrects are the sensing path's"),
    (("filter", "observe", "adapt"), "mpc: filter= together with adapt= is refused: the adaptive controller traces the plant's "
                                     "exact state"),
    (("filter", "observe", "policy"), "mpc: filter= together with policy= is refused: the policy's memory is forked from the "
                                      "plant's exact state"),
    (("observe", "adapt"), "mpc: observe= together with adapt= is refused: the adaptive controller traces the plant's exact "
                           "state"),
    (("observe", "policy"), "mpc: observe= together with policy= is refused: the policy's memory is forked from the plant's "
                            "exact state"),
    (("terminal_value", "!policy"), "mpc: terminal_value needs policy=<checkpoint>: the critic is the policy's"),
    (("policy", "adapt"), "mpc: policy= together with adapt= is refused: the adaptive controller does not roll the policy yet"),
)
# more keys than one entry names: the entry that won before wins now
RECORDED_BEYOND = (
    (("filter", "adapt"), RECORDED[5][1]),
    (("filter", "policy"), RECORDED[5][1]),
    (("track", "observe", "policy"), RECORDED[1][1]),
    (("track", "observe", "filter"), RECORDED[3][1]),
    (("track", "filter", "adapt"), RECORDED[2][1]),
    (("observe", "policy", "adapt"), RECORDED[8][1]),
)
ARGUMENT = {"track": {"PATH": "exact"}, "observe": {"DELAY": 1}, "filter": {}, "adapt": {"params": {"DAMPING": [0.005, 0.1]}},
            "policy": "x.pth", "terminal_value": 1.0}


def _play_with_exactly(keys, monkeypatch):
    """``mpc.play`` with the keywords ``keys`` name and no other; making a task is an error."""
    def no_task(*a, **k):
        raise AssertionError("a task was made before the combination was refused")

    monkeypatch.setattr(mpc, "make_task", no_task)
    env = {"numEnvs": 2}
    if "track" in keys and "!ENV_TARGET" not in keys:
        env["ENV_TARGET"] = {"VEL_ALONG": 0.1, "SPAN_ALONG": 0.05}
    return mpc.play({"env": env, "seed": 0}, samples=256, **{k: ARGUMENT[k] for k in keys if not k.startswith("!")})


def test_rule_table_has_the_recorded_keys_in_the_recorded_order():
    assert [keys for keys, _ in mpc.RULES] == [keys for keys, _ in RECORDED]


@pytest.mark.parametrize("index", range(len(RECORDED)))
def test_play_refuses_every_entry_of_the_rule_table_with_the_recorded_message(index, monkeypatch):
    keys = mpc.RULES[index][0]
    with pytest.raises(ConfigError) as e:
        _play_with_exactly(keys, monkeypatch)
    assert str(e.value) == RECORDED[index][1]


@pytest.mark.parametrize("keys,message", RECORDED_BEYOND)
def test_play_keeps_the_winner_where_several_rules_apply(keys, message, monkeypatch):
    with pytest.raises(ConfigError) as e:
        _play_with_exactly(keys, monkeypatch)
    assert str(e.value) == message


# ---- the run loop
H, W = 5, 2      # model steps per control step, and per adapt pass


class _Task:
    def __init__(self):
        self.num_steps, self.step_count, self.replays = 0, 0, []

    def live_tensors(self):
        return []

    def observers_replayed(self, n_steps, before=False):
        if not before:
            self.replays.append(n_steps)


class _Graph:
    """What ``capture_rolled_back`` returns here: a replay moves the controller's position on by the unit."""

    def __init__(self, ctl):
        self.ctl = ctl

    def replay(self):
        self.ctl.events.append("replay")
        self.ctl.position += self.ctl.unit_steps


def _stub(cls, unit_steps, use_graph, tasks=2):
    """An instance of ``cls`` with no device: the counters ``Controller.__init__`` leaves and stubbed launches."""
    ctl = cls.__new__(cls)
    ctl.tasks = tuple(_Task() for _ in range(tasks))
    ctl.plant, ctl.model = ctl.tasks[:2]
    ctl.device, ctl.graph, ctl.use_graph = None, None, use_graph
    ctl.unit_steps = ctl.graph_steps = unit_steps
    ctl.launches = {"step": 0, "plant_step": 0, "anchor": 0, "trace": 0, "adapt_step": 0}
    ctl.control_steps, ctl.position, ctl.events, ctl.capturing = 0, 0, [], False
    return ctl


def _count(ctl, event, **launches):
    if not ctl.capturing:
        ctl.events.append(event)
    for k, v in launches.items():
        ctl.launches[k] += v


class _Steps(mpc.Controller):
    """A unit of ``unit_steps`` control steps; a boundary wherever the position is a multiple of it."""

    def tensors(self):
        return []

    def control_step(self):
        _count(self, "step", step=H, plant_step=1)
        self.plant.num_steps += 1
        self.model.num_steps += H
        for extra in self.tasks[2:]:          # a third task that steps twice per control step, as a predictor would
            extra.num_steps += 2
        if not self.capturing:
            self.position += 1

    def at_boundary(self):
        return self.position % self.unit_steps == 0


class _Cycles(mpc_adapt.AdaptiveController):
    """``AdaptiveController``'s own unit, boundary and eager step over stubbed launches."""

    def tensors(self):
        return []

    def anchor(self):
        _count(self, "anchor", anchor=1)

    def trace(self):
        _count(self, "trace", trace=1)

    def control_step(self):
        _count(self, "step", step=H, plant_step=1)
        self.plant.num_steps += 1
        self.model.num_steps += H

    def adapt_pass(self):
        _count(self, "adapt", adapt_step=W)
        self.model.num_steps += W


@pytest.fixture
def fake_capture(monkeypatch):
    """``capture_rolled_back`` as the host sees it: the body runs twice, nothing of the device is touched."""
    def capture(device, body, live, env, pool=None):
        ctl = body.__self__
        before, ctl.capturing = env.step_count, True
        body()
        body()
        env.step_count, ctl.capturing = before, False
        return _Graph(ctl)

    monkeypatch.setattr(graph_capture, "capture_rolled_back", capture)


def _totals(ctl):
    return ctl.control_steps, ctl.launches, [t.num_steps for t in ctl.tasks]


@pytest.mark.parametrize("tasks", (2, 3))
def test_run_replays_whole_units_from_a_boundary_and_steps_eagerly_elsewhere(fake_capture, tasks):
    ctl, eager = _stub(_Steps, 3, True, tasks), _stub(_Steps, 3, False, tasks)
    ctl.run(10)
    assert ctl.events == ["replay"] * 3 + ["step"]
    assert ctl.graph_launches == {"step": 3 * H, "plant_step": 3, "anchor": 0, "trace": 0, "adapt_step": 0}
    assert ctl.graph_num_steps == [3, 3 * H, 6][:tasks]
    assert ctl.plant.replays == [3, 3, 3]
    eager.run(10)
    assert eager.events == ["step"] * 10
    assert _totals(ctl) == _totals(eager) == (10, {"step": 10 * H, "plant_step": 10, "anchor": 0, "trace": 0, "adapt_step": 0},
                                              [10, 10 * H, 20][:tasks])
    # off a boundary: eager steps until one is reached, then replays, then what is left
    ctl.events.clear()
    ctl.run(10)
    assert ctl.position == 20 and ctl.events == ["step"] * 2 + ["replay"] * 2 + ["step"] * 2
    eager.run(10)
    assert _totals(ctl) == _totals(eager) and ctl.control_steps == 20 and ctl.plant.num_steps == 20
    # less than a unit is never a replay, and captures nothing
    short = _stub(_Steps, 3, True)
    short.run(2)
    assert short.graph is None and short.events == ["step"] * 2


def test_adaptive_run_keeps_the_interleaving_of_cycles_and_eager_steps(fake_capture):
    E = 4

    def make(use_graph):
        ctl = _stub(_Cycles, E, use_graph)
        ctl.E, ctl.graph_cycles, ctl.phase = E, 1, 0
        return ctl

    ctl, eager = make(True), make(False)
    one = ["step", "trace"]
    ctl.run(3)
    assert ctl.events == ["anchor"] + one * 3 and ctl.phase == 3 and ctl.graph is None
    ctl.events.clear()
    ctl.run(6)         # the running cycle's last step and its pass, one whole cycle from the graph, the next one's first step
    assert ctl.events == one + ["adapt", "replay", "anchor"] + one and ctl.phase == 1
    assert ctl.graph_launches == {"step": E * H, "plant_step": E, "anchor": 1, "trace": E, "adapt_step": W}
    assert ctl.graph_num_steps == [E, E * H + W] and ctl.plant.replays == [E]
    ctl.events.clear()
    ctl.run(4)         # never on a boundary with a whole cycle left: all eager
    assert ctl.events == one * 3 + ["adapt", "anchor"] + one and ctl.phase == 1
    for n in (3, 6, 4):
        eager.run(n)
    assert "replay" not in eager.events and eager.phase == 1
    assert _totals(ctl) == _totals(eager) == (13, {"step": 13 * H, "plant_step": 13, "anchor": 4, "trace": 13, "adapt_step": 3 * W},
                                              [13, 13 * H + 3 * W])
