"""Capture of a hipGraph whose body steps the env: warm up on a side stream, roll everything back, then capture.

The warm-up pass executes the body once outside capture (lazy initialisations of libraries, autotuning); its effects are
rolled back, and the capture pass executes nothing.  So neither pass counts towards the env's step observers
(utils/observers.py): both run under ``env.observers_paused()``, and every replay is bracketed by ``replay_observed``.
What is rolled back is the caller's own tensors and ``env.live_tensors()`` -- the env's buffers and what each of its
observers says it needs --, the env's step count (the key of the random streams) and the device RNG state."""
import contextlib
import gc

import torch


@contextlib.contextmanager
def collector_at_rest():
    """Around a stream capture: dead reference cycles are collected in front of it and the cyclic collector rests during it.
    A cycle may own an env handle or a ``torch.cuda.CUDAGraph`` (a closed-over agent of an earlier run in the same process),
    and their finalisers synchronise the device and free device memory.  The collector starts wherever an allocation tips
    it over, on whichever thread -- the autograd thread of a captured backward pass included --, and such a finaliser run
    inside a capture ends the process (abort).  (``torch.cuda.graph`` itself collects on entry only under
    ``torch.compiler.config.force_cudagraph_gc``, and never keeps the collector from starting later.)"""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def capture_rolled_back(device, body, live, env, pool=None):
    """``body()`` captured as a ``torch.cuda.CUDAGraph``.  ``live``: every tensor the body writes that must read after the
    capture as before it: the caller's own, concatenated with ``env.live_tensors()``."""
    paused = getattr(env, "observers_paused", contextlib.nullcontext)      # (an env without the observers API)
    backup = [t.clone() for t in live]
    step, rng = env.step_count, torch.cuda.get_rng_state(device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side), paused():
        body()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    for t, b in zip(live, backup):
        t.copy_(b)
    env.step_count = step
    torch.cuda.set_rng_state(rng, device)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    # thread_local: RCCL's watchdog thread may touch the HIP runtime while this thread captures
    with collector_at_rest(), torch.cuda.graph(graph, pool=pool, capture_error_mode="thread_local"), paused():
        body()
    return graph


def replay_observed(graph, env, n_steps):
    """Replay a graph holding ``n_steps`` env steps, telling the env's observers of them before and after."""
    replayed = getattr(env, "observers_replayed", None)
    if replayed is not None:
        replayed(n_steps, before=True)
    graph.replay()
    if replayed is not None:
        replayed(n_steps)
