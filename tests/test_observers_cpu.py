"""The step-observer protocol (utils/observers.py) without a GPU: every observer class defines every name of it, and the
schedule function has one definition."""
import inspect

import pytest

from vine_robot_isaacgymenvs_amd.utils import observers, video
from vine_robot_isaacgymenvs_amd.utils.episodes import EpisodeLog
from vine_robot_isaacgymenvs_amd.utils.trajectory import TrajectoryRecorder
from vine_robot_isaacgymenvs_amd.utils.video import VideoCapture

METHODS = ("before", "enqueue", "advance", "set_steps", "live_tensors", "drain", "close")
ATTRIBUTES = ("paused", "copy_done")


def _constructor_names(cls):
    """The names the constructors of ``cls`` and its bases mention: an attribute they set is among them."""
    names = set()
    for base in cls.__mro__[:-1]:               # (object has no Python constructor)
        init = base.__dict__.get("__init__")
        if init is not None:
            names.update(init.__code__.co_names)
    return names


@pytest.mark.parametrize("cls", [VideoCapture, TrajectoryRecorder, EpisodeLog])
def test_observer_defines_the_protocol(cls):
    for name in METHODS:
        fn = inspect.getattr_static(cls, name, None)
        assert inspect.isfunction(fn), (cls.__name__, name)
    sig = inspect.signature(cls.enqueue)
    assert list(sig.parameters)[:3] == ["self", "stream", "actions"]
    for name in ("before", "advance", "set_steps"):
        assert len(inspect.signature(getattr(cls, name)).parameters) == 2, (cls.__name__, name)
    for name in ("live_tensors", "drain", "close"):
        assert len(inspect.signature(getattr(cls, name)).parameters) == 1, (cls.__name__, name)
    assert set(ATTRIBUTES) <= _constructor_names(cls), cls.__name__
    for name in METHODS + ATTRIBUTES:            # and the module docstring states each of them
        assert name in observers.__doc__, name


def test_windowed_observers_share_the_harvest():
    shared = ("set_steps", "before", "advance", "_skip", "_harvest", "_write_loop", "drain", "close")
    for cls in (VideoCapture, TrajectoryRecorder):
        assert issubclass(cls, observers.WindowRing)
        for name in shared:
            assert name not in cls.__dict__, (cls.__name__, name)
        for name in ("enqueue", "live_tensors", "_window", "_copies", "_write"):
            assert name in cls.__dict__, (cls.__name__, name)
    assert not issubclass(EpisodeLog, observers.WindowRing)


def test_capture_schedule_has_one_definition():
    from vine_robot_isaacgymenvs_amd.utils.observers import capture_schedule as a
    from vine_robot_isaacgymenvs_amd.utils.video import capture_schedule as b
    assert a is b and a.__module__ == observers.__name__
    assert video.capture_schedule is observers.capture_schedule
