"""StepGraph — closed-loop steps of a BatchedTradingEnv replayed as ONE HIP graph.

A small batch is launch-bound, not bandwidth-bound: config 2 (4 096 envs, 1 MB per step) spends
more time between two launches than inside the kernel.  Everything `gte_step` enqueues is
stream-capturable (device-resident actions), so the steps — and whatever torch code produces the
actions between them: a policy forward pass — can be recorded once with `torch.cuda.graph` and
replayed with one host call per K steps.

    g = env.capture_steps(lambda i: env.step(policy(env._t["obs"])), n_steps=64)
    for _ in range(1000):
        g.replay()          # 64 env steps (and 64 policy calls) per host call

Envs with a trajectory log — `log_steps`, or a Python `reward_function` / dynamic feature, which
bring one — are captured too: the log's row count lives on the device (gte.h, gte_log_view.cursor),
so every replay appends its rows where the log is and the captured `BatchedHistory` reads pick
their rows there (batched_history.py).  The log must be full before the capture (take `log_steps`
eager steps first).  The host's own schedule (terminal-counter slot, log row count, steps since the
last re-sort) is saved before the capture and put back after it — a capture runs nothing, and a
body that raised leaves the env as it was — and each replay advances the host's row count by the
rows it appended.  The captured graph is one linear chain on one side stream.

The L2-affinity re-sorts (`affinity_period`) are captured where they fell during the capture: a
graph replays them at those steps whatever the env's count is at replay time, so a graph shorter
than the period re-sorts on a fixed schedule of its own (results do not depend on the order).

Results are those of the same eager calls, bit for bit (tests/test_gpu_graph.py,
tests/test_gpu_graph_log.py).
"""
from __future__ import annotations

import ctypes as C

from . import _abi


class StepGraph:
    def __init__(self, env, body, n_steps: int):
        torch = env._torch
        if torch is None:
            raise ValueError("capture_steps needs output='torch' (the steps run on a torch stream)")
        if n_steps < 2 or n_steps % 2:
            # the two-slot terminal counter alternates per launch (gte.h, gte_step): after an even
            # number of steps a replay leaves it where the capture found it
            raise ValueError("n_steps must be even and >= 2")
        if env.return_slots != 1:
            raise ValueError("capture_steps needs return_slots=1 (the rotation is host state)")
        L = int(env.cfg.log_steps)
        if L and env._log_view().rows < L:
            # a full log keeps len(history) the same in every replay
            raise ValueError(f"capture_steps with a trajectory log needs a full log: take log_steps = {L} "
                             f"eager steps (reset included) first, {int(env._logv.rows)} rows are logged")
        self.env, self.n_steps = env, int(n_steps)
        dev = env._t["obs"].device
        if L and env._log_back is None:  # made outside the capture
            env._log_back = torch.arange(-L, 0, device=dev)
        saved = self._schedule()
        self._slot = int(saved.term_slot)
        home = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(home)
        self._set_stream(side)  # (synchronises the env's previous stream: before the capture starts)
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph, stream=side):
                for i in range(self.n_steps):
                    body(i)
        finally:
            self._set_stream(home)
            # capturing enqueued nothing: the host schedule goes back to where the capture found it
            captured = self._schedule()
            _abi.check(env._lib, env._lib.gte_set_schedule(env._h, C.byref(saved)))
            env._epoch += 1
        if captured.term_slot != saved.term_slot:
            raise RuntimeError("the captured body did not take an even number of env steps")
        self._log_rows = int(captured.log_rows - saved.log_rows)  # appended by each replay

    def _schedule(self):
        e, s = self.env, _abi.GteSchedule()
        _abi.check(e._lib, e._lib.gte_get_schedule(e._h, C.byref(s)))
        return s

    def _term_slot(self) -> int:
        e = self.env
        _abi.check(e._lib, e._lib.gte_get_outputs(e._h, C.byref(e._out)))
        return int(e._out.term_slot)

    def _set_stream(self, stream):
        e = self.env
        _abi.check(e._lib, e._lib.gte_set_stream(e._h, C.c_void_p(stream.cuda_stream)))

    def replay(self):
        """Run the captured steps once more on torch's current stream."""
        if self._term_slot() != self._slot:
            raise RuntimeError("an odd number of eager steps was taken since the capture: the graph's "
                               "terminal-counter slots no longer match (take one more eager step, or "
                               "capture again)")
        self.graph.replay()
        if self._log_rows:  # the host's count of the log rows follows the device cursor
            _abi.check(self.env._lib, self.env._lib.gte_advance_log(self.env._h, self._log_rows))
        self.env._epoch += 1  # state snapshots / info caches of earlier steps are stale
