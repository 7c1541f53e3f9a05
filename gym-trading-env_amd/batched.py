"""BatchedTradingEnv — N reference-semantics TradingEnvs stepped by one HIP launch.

Host-side mirror of the reference's `TradingEnv` surface
(src/gym_trading_env/environments.py:79-125 constructor, :163 reset, :233 step)
for a batch: same argument names and meaning, same asserts, `step(actions)`
returning `(obs, reward, terminated, truncated, info)`.  All arithmetic happens
in libgte's kernels (csrc/); this file only stages data, marshals pointers and
wraps device buffers.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, spaces, staging
from .batched_history import history_column, history_columns
from .config import make_config

_NP = {"int32": np.int32, "float64": np.float64}


def _as_staged(ds, n_dyn, name="Stock"):
    if isinstance(ds, staging.StagedDataset):
        return ds
    if isinstance(ds, tuple) and len(ds) in (2, 4):  # (features, close[, high, low])
        return staging.stage_arrays(ds[0], ds[1], n_dyn=n_dyn, name=name,
                                    high=ds[2] if len(ds) == 4 else None,
                                    low=ds[3] if len(ds) == 4 else None)
    return staging.stage_dataframe(ds, n_dyn=n_dyn, name=name)  # a pandas DataFrame


def _device_view(ptr, shape, typestr, device, strides=None):
    """torch view of device memory at `ptr` (no copy), through the CUDA array interface
    torch.as_tensor understands (also on ROCm)."""
    import torch

    class _Raw:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "version": 2,
                                    "strides": strides, "data": (int(ptr), False)}
    return torch.as_tensor(_Raw(), device=device)


def info_column(env, key, final: bool = False) -> np.ndarray:
    """`info[key]` for every env, on the host: History column `key` of the current state or
    (final) of the terminal records, with the last step's f64 reward."""
    state = env.final_state if final else env.state
    return history_column(key, lambda f: env.read_output("reward64") if f == "reward" else state(f),
                          np.asarray(env.positions, dtype=np.float64), env)


class LazyInfo(dict):
    """`info` of a batched step: struct-of-arrays view of what the reference logs in
    `History` each step and returns as `history[-1]` (environments.py:253-264, :272), fetched
    from HBM only on access, one host array of length N per key.

    Keys are History's flattened column names (docs/source/history.rst:18-46,
    docs/source/vectorize_env.rst:25-33): idx, step, date, position_index, position,
    real_position, data_<every non-feature column of the DataFrame>, portfolio_valuation,
    portfolio_distribution_{asset,fiat,borrowed_asset,borrowed_fiat,interest_asset,
    interest_fiat}, reward — plus dataset_index.  `_key` is Gymnasium's presence mask (all True).
    With ``autoreset="same_step", final_obs=True`` the envs whose episode ended in this step
    also get Gymnasium's `final_observation` / `final_info` (object arrays, `None` elsewhere)
    with their `_final_observation` / `_final_info` masks."""

    def __init__(self, env):
        super().__init__()
        self._env = env
        self._KEYS = tuple(env.info_keys)
        self._final = bool(env.cfg.final_obs)

    def keys(self):
        return list(self._KEYS) + (["final_observation", "final_info"] if self._final else [])

    def __contains__(self, k):
        return k in self._KEYS or (self._final and k in ("final_observation", "final_info",
                                                         "_final_observation", "_final_info")) \
            or (isinstance(k, str) and k.startswith("_") and k[1:] in self._KEYS)

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def __missing__(self, key):
        e = self._env
        if self._final and key in ("final_observation", "final_info", "_final_observation",
                                   "_final_info"):
            self.update(e._final_entries())
            return dict.__getitem__(self, key)
        if key.startswith("_") and key[1:] in self._KEYS:
            # Gymnasium's vector-env convention (docs/source/vectorize_env.rst:25-33): `_key`
            # marks the envs for which `key` is present — here always all of them
            v = np.ones(e.num_envs, dtype=bool)
        elif key in self._KEYS:
            v = info_column(e, key)
        else:
            raise KeyError(key)
        self[key] = v
        return v


try:  # soft dependency: lets `isinstance(env, gymnasium.vector.VectorEnv)` hold
    from gymnasium.vector import VectorEnv as _VectorEnvBase  # type: ignore
except Exception:
    _VectorEnvBase = object


class BatchedTradingEnv(_VectorEnvBase):
    """N independent trading environments resident in HBM.

    Follows Gymnasium's vector-env conventions (docs/source/vectorize_env.rst:17-33):
    `num_envs`, `single_observation_space` / `single_action_space`, batched
    `observation_space` / `action_space`, `reset() -> (obs, info)`, `step(actions) ->
    (obs, rewards, terminations, truncations, infos)` with dict-of-arrays infos and `_key`
    masks, auto-reset in next-step (Gymnasium >= 1.0) or same-step mode.

    Parameters mirror `TradingEnv.__init__` (environments.py:79-93); the extra ones:

    :param df: one dataset or a list of datasets: pandas DataFrames (feature columns
        contain "feature", a "close" column), ``StagedDataset`` objects, or
        ``(features[T, F_s], close[T][, high[T], low[T]])`` tuples.  Several datasets give the
        `MultiDatasetTradingEnv` behaviour (:365-400) with all of them resident.
    :param num_envs: N.
    :param autoreset: None/"disabled", "next_step" (Gymnasium >= 1.0) or "same_step".
    :param output: "torch" — observations/rewards/flags stay on the device as torch
        tensors (zero-copy views of the buffers the kernel writes); "numpy" — copied to
        host each step (compatibility mode).
:param final_obs: with ``autoreset="same_step"``: keep the terminal observation of
        every env that ends (Gymnasium's ``final_observation`` / SB3's
        ``terminal_observation``); read it with :meth:`final_observations`.
:param log_steps: L > 0 keeps the last L steps of every env in a device trajectory
        log; :meth:`history` turns one env's episode into a `History` (the object the
        reference hands to custom reward / metric functions) and `add_metric` functions
        are evaluated by :meth:`episode_metrics`.
    :param dyn_persist: keep the per-env dynamic-feature column across episodes like
        the reference's in-place write into `_obs_array` (:153-154); costs
        N*T*n_dyn*4 bytes of HBM.
    """

    metadata = {"render_modes": ["logs"]}

    def __init__(self, df, num_envs: int, positions=(0, 1),
                 dynamic_feature_functions=("last_position_taken", "real_position"),
                 reward_function="basic_reward_function", windows=None, trading_fees=0,
                 borrow_interest_rate=0, portfolio_initial_value=1000,
                 initial_position="random", max_episode_duration="max", verbose=1,
                 name="Stock", render_mode="logs", *, autoreset="next_step",
                 episodes_between_dataset_switch=1, dyn_persist=False, seed=0,
                 env_id_base=0, device=0, output="torch", envs_per_wave=0,
                 nontemporal_obs=3, kernel_variant=0, library_path=None, debug_flags=0,
                 affinity_period=0, final_obs=False, log_steps=0, return_slots=1, copy=True,
                 obs_slack_rows=0):
        assert render_mode is None or render_mode in self.metadata["render_modes"]
        if output not in ("torch", "numpy"):
            raise ValueError("output must be 'torch' or 'numpy'")
        self.positions = list(positions)
        self.windows = windows
        self.verbose, self.name, self.render_mode = verbose, name, render_mode
        self.num_envs = int(num_envs)
        self.output = output
        # return_slots=K > 1 (torch output): step t writes reward/terminated/truncated into
        # row t % K of one [K, 6N] buffer, so a collective still reading older returns is not
        # overwritten by the next K-1 steps, and runs of consecutive steps are contiguous
        # blocks (distributed.ReturnPipeline gathers them a block at a time)
        # copy=False (output="numpy", Gymnasium's vector-env convention): step()/reset() return
        # views of the library's pinned staging buffer, overwritten by the next call — no
        # 168 MB allocation + copy per step at the headline shape
        self.copy = bool(copy)
        # verbose > 0 with a trajectory log the USER asked for: the reference's episode-end line
        # (environments.py:269-271, :289-294) for the envs that finished — at most
        # `verbose_max_lines` per report and one report per `verbose_interval` seconds (a report
        # costs a device synchronisation; 0 = after every step)
        self.verbose_max_lines = 16
        self.verbose_interval = 1.0
        self._last_report = 0.0
        self._user_log = int(log_steps) > 0
        self.return_slots = int(return_slots)
        if self.return_slots < 1 or (self.return_slots > 1 and output != "torch"):
            raise ValueError("return_slots must be >= 1 (and > 1 only with output='torch')")
        mode = autoreset or "disabled"
        try:  # Gymnasium >= 1.0 wrappers read an AutoresetMode enum here (unpinned: not installed here)
            from gymnasium.vector import AutoresetMode  # type: ignore
            mode = {"next_step": AutoresetMode.NEXT_STEP, "same_step": AutoresetMode.SAME_STEP,
                    "disabled": AutoresetMode.DISABLED}[mode]
        except Exception:  # noqa: BLE001
            pass
        self.metadata = dict(self.metadata, autoreset_mode=mode)
        self.closed = False
        self._lib = _abi.load_library(library_path)  # raises if the HIP build is missing
        self._h = C.c_void_p()

        from .config import HOST_CALLABLE, resolve_dynamic_features, resolve_reward
        dyn_kinds = resolve_dynamic_features(dynamic_feature_functions)
        n_dyn = len(dyn_kinds)
        # a user's own callables (anything but this package's default objects / the string and
        # tuple specs) are evaluated after every launch, vectorised over a BatchedHistory
        self._dyn_callables = [(i, f) for i, (k, f) in enumerate(zip(dyn_kinds, dynamic_feature_functions))
                               if k == HOST_CALLABLE]
        self._reward_callable = (reward_function if resolve_reward(reward_function)[0] == HOST_CALLABLE
                                 else None)
        if self._dyn_callables or self._reward_callable is not None:
            if output != "torch":
                raise NotImplementedError("custom reward / dynamic-feature callables in the batch are "
                                          "evaluated on the device: use output='torch'")
            if autoreset == "same_step":
                final_obs = True  # the terminal History row of an env that ends comes from its terminal record
            log_steps = max(int(log_steps), 2)  # the callables read h[..., -1] and h[..., -2]
        raw = list(df) if isinstance(df, (list, tuple)) and not (
            isinstance(df, tuple) and len(df) in (2, 4) and hasattr(df[0], "shape")) else [df]
        self.datasets = [_as_staged(d, n_dyn, name) for d in raw]
        first = self.datasets[0]
        for d in self.datasets:
            if d.n_static != first.n_static or d.n_dyn != n_dyn:
                raise ValueError("all datasets must have the same feature columns")
            staging.check_episode_geometry(d.T, windows, max_episode_duration)

        self.cfg = make_config(
            n_envs=self.num_envs, n_static=first.n_static, n_datasets=len(self.datasets),
            positions=self.positions, dynamic_feature_functions=dynamic_feature_functions,
            reward_function=reward_function, windows=windows, trading_fees=trading_fees,
            borrow_interest_rate=borrow_interest_rate,
            portfolio_initial_value=portfolio_initial_value,
            initial_position=initial_position, max_episode_duration=max_episode_duration,
            autoreset=autoreset, episodes_between_dataset_switch=episodes_between_dataset_switch,
            dyn_persist=dyn_persist, seed=seed, env_id_base=env_id_base, device=device,
            envs_per_wave=envs_per_wave, nontemporal_obs=nontemporal_obs,
            kernel_variant=kernel_variant, debug_flags=debug_flags,
            affinity_period=affinity_period, final_obs=final_obs, log_steps=log_steps,
            obs_slack_rows=obs_slack_rows)
        self.log_metrics = []
        self.info_keys = history_columns(self) + ["dataset_index"]
        self._ds_offsets = np.concatenate([[0], np.cumsum([d.T for d in self.datasets])]).astype(np.int64)
        self._host_columns, self._dev_columns = {}, {}
        _abi.check(self._lib, self._lib.gte_create(C.byref(self.cfg), C.byref(self._h)))

        self.n_obs = first.n_static + n_dyn
        self.obs_shape = (self.n_obs,) if windows is None else (int(windows), self.n_obs)
        # environments.py:112-123
        self.single_action_space = spaces.Discrete(len(self.positions))
        self.single_observation_space = spaces.Box(-np.inf, np.inf, shape=self.obs_shape)
        self.action_space = spaces.MultiDiscrete([len(self.positions)] * self.num_envs)
        self.observation_space = spaces.Box(-np.inf, np.inf,
                                            shape=(self.num_envs,) + self.obs_shape)
        self._signals = {}  # dataset -> the padded int8 [S, stride] device tensor bound to it (bind_signals)
        self._backtest_map = None  # (strategy tensor or None, S) of the last backtest_signals(); None after backtest()
        self._exits = None  # (rules tensor, rule_of_env tensor or None) bound by bind_exits, kept alive
        self._exit_state_ptr = 0  # device address of the exit states (0 before the first bind_exits)
        self._trades_ptr = 0  # device address of the trade records while track_trades() is on, else 0
        self._trade_list_capacity = 0  # capacity of the trade list while track_trades(list_capacity=...) keeps one
        # (device address of the period records, B, their generation) while track_periods() is on, else None; the
        # generation counts the allocations: a PeriodStats of an earlier one views freed memory and must refuse
        self._periods = None
        self._period_records, self._period_generation = None, 0
        for d, s in enumerate(self.datasets):
            self.upload_dataset(d, s)

        self._logv, self._log_tensors = _abi.GteLogView(), {}
        self._log_cursor = None  # torch view of gte_log_view.cursor (i64 [2]), made on first need
        self._log_back = None    # arange(-L, 0) on the device, made before a capture (StepGraph)
        # state snapshots, taken lazily: [view, epoch] of the current state and of the terminal records
        self._snapshots = {False: [_abi.GteStateView(), -1], True: [_abi.GteStateView(), -1]}
        self._snapshot_tensors = {}  # torch views of the snapshots, by (final, name)
        self._epoch = 0
        self._snap_epoch, self._snap, self._snap_obs = -1, None, None  # numpy mode, per step
        self._torch = None
        self._t = {}
        # sliding observation buffer (torch output, where the library grants it): [N, W + M, F_obs] and
        # its M + 1 window views, one per head; _t["obs"] is the view at the library's current head
        self._obs_slab, self._obs_views, self._obs_view = None, None, _abi.GteObsView()
        if output == "torch":
            self._bind_torch_outputs()
        # the values `position` takes, on the device in torch mode
        self._pos_table = np.asarray(self.positions, dtype=np.float64) if self._torch is None else \
            self._torch.tensor(self.positions, dtype=self._torch.float64, device=self._t["obs"].device)
        self._out = _abi.GteOutputs()
        _abi.check(self._lib, self._lib.gte_get_outputs(self._h, C.byref(self._out)))
        self._was_reset = False
        if _VectorEnvBase is not object:
            # gymnasium installed: run the base initialiser too (unpinned — gymnasium is not in the
            # build / test images; >= 1.0 takes no arguments, 0.29 takes the three below), then put
            # this class's own spaces back
            keep = (self.observation_space, self.action_space)
            try:
                try:
                    _VectorEnvBase.__init__(self)
                except TypeError:
                    _VectorEnvBase.__init__(self, self.num_envs, self.single_observation_space,
                                            self.single_action_space)
            except Exception:  # noqa: BLE001 - never let an optional base class break the env
                pass
            self.observation_space, self.action_space = keep

    @classmethod
    def from_dataset_dir(cls, dataset_dir: str, num_envs: int, *args,
                         preprocess=lambda df: df, episodes_between_dataset_switch: int = 1,
                         **kwargs):
        """The batched `MultiDatasetTradingEnv` (environments.py:365-400): every file matched
        by the glob `dataset_dir` is loaded (`pd.read_pickle`), passed through `preprocess`
        and kept RESIDENT in HBM; each env moves to another dataset every
        `episodes_between_dataset_switch` episodes, visiting all of them once per round of
        D picks in uniformly random order: each pick is uniform among the datasets the round
        has not visited yet (== uniform among the least-used ones, :383-388)."""
        import glob
        from pathlib import Path

        import pandas as pd
        paths = glob.glob(dataset_dir)
        if len(paths) == 0:  # :376
            raise FileNotFoundError(f"No dataset found with the path : {dataset_dir}")
        frames = [preprocess(pd.read_pickle(p)) for p in paths]  # the user's own dataset files
        env = cls(frames, num_envs, *args,
                  episodes_between_dataset_switch=episodes_between_dataset_switch, **kwargs)
        env.dataset_pathes = paths
        env.dataset_names = [Path(p).name for p in paths]
        return env

    # -- setup ---------------------------------------------------------------------
    def upload_dataset(self, d: int, s: staging.StagedDataset):
        """`_set_df` (environments.py:128-143): stage one dataset into HBM."""
        feat = np.ascontiguousarray(s.feat, dtype=np.float32)
        close = np.ascontiguousarray(s.close, dtype=np.float64)
        ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data
        _abi.check(self._lib, self._lib.gte_upload_dataset(
            self._h, d, feat.ctypes.data, close.ctypes.data, ptr(s.high), ptr(s.low), s.T))
        self.datasets[d] = s
        self._signals.pop(d, None)  # (the library unbound the dataset's signal table: T may differ)

    def _bind_torch_outputs(self):
        import torch
        if not torch.cuda.is_available():
            raise _abi.GteError(_abi.GTE_ERR_NO_DEVICE, "torch sees no GPU; there is no CPU fallback")
        self._torch = torch
        dev = torch.device("cuda", self.cfg.device)
        N = self.num_envs
        with torch.cuda.device(dev):
            # reward | terminated | truncated live in ONE buffer (distributed.packed_layout)
            # so that a sharded run all-gathers it without a packing kernel
            self._packed_all = torch.zeros((self.return_slots, 6 * N), dtype=torch.uint8,
                                           device=dev)
            self._packed = list(self._packed_all.unbind(0))
            # per slot, made once: the buffer, its (reward, terminated, truncated) views and
            # the three device pointers gte_bind_returns takes
            self._slot_views = []
            for buf in self._packed:
                base = buf.data_ptr()
                self._slot_views.append((
                    buf,
                    (buf[:4 * N].view(torch.float32), buf[4 * N:5 * N].view(torch.bool),
                     buf[5 * N:].view(torch.bool)),
                    (C.c_void_p(base), C.c_void_p(base + 4 * N), C.c_void_p(base + 5 * N))))
            # outputs start bound to row 0 (reset writes there); the first step rotates to it
            self._ret_slot = self.return_slots - 1
            self.packed_returns = self._packed[0]
            # obs: a sliding buffer where the library grants one (gte.h, gte_bind_sliding_obs), bound below
            _abi.check(self._lib, self._lib.gte_obs_view(self._h, C.byref(self._obs_view)))
            M = int(self._obs_view.slack_rows)
            if M > 0:
                W, F = self.obs_shape
                self._obs_slab = torch.zeros((N, W + M, F), dtype=torch.float32, device=dev)
                self._obs_views = [self._obs_slab[:, h:h + W, :] for h in range(M + 1)]
            self._t = {
                "obs": self._obs_views[0] if M > 0 else
                torch.zeros((N,) + self.obs_shape, dtype=torch.float32, device=dev),
                "reward": self.packed_returns[:4 * N].view(torch.float32),
                "reward64": torch.zeros(N, dtype=torch.float64, device=dev),
                "terminated": self.packed_returns[4 * N:5 * N].view(torch.bool),
                "truncated": self.packed_returns[5 * N:].view(torch.bool),
                "term_count": torch.zeros(2, dtype=torch.int32, device=dev),  # two slots
                "term_ids": torch.zeros(N, dtype=torch.int32, device=dev),
            }
            if self.cfg.final_obs:
                self._t["final_obs"] = torch.zeros((N,) + self.obs_shape, dtype=torch.float32,
                                                   device=dev)
            torch.cuda.synchronize(dev)
            b = _abi.GteOutputs()
            for k, t in self._t.items():
                setattr(b, k, t.data_ptr())
            if M > 0:  # (the slab's start, so that the library allocates no buffer of its own meanwhile)
                b.obs = self._obs_slab.data_ptr()
            _abi.check(self._lib, self._lib.gte_bind_outputs(self._h, C.byref(b)))
            if M > 0:
                _abi.check(self._lib, self._lib.gte_bind_sliding_obs(
                    self._h, C.c_void_p(self._obs_slab.data_ptr()), self.obs_shape[0] + M))
            # run on torch's current stream so torch ops and env launches are ordered
            _abi.check(self._lib, self._lib.gte_set_stream(
                self._h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    # -- sliding observation buffer ---------------------------------------------------
    @property
    def sliding_obs(self) -> bool:
        """True while observations live in a sliding buffer: `obs` is then a strided view
        [N, W, F_obs] of a [N, W + M, F_obs] tensor (contiguous within an env, chronological)."""
        return self._obs_views is not None

    def _follow_head(self):
        """_t["obs"] = the window at the library's head (after every reset, step and rollout)."""
        v = self._obs_view
        _abi.check(self._lib, self._lib.gte_obs_view(self._h, C.byref(v)))
        if v.sliding:
            self._t["obs"] = self._obs_views[v.head]
        else:  # somebody bound a classic buffer through the C ABI: follow it for good
            self._t["obs"] = _device_view(v.base, (self.num_envs,) + self.obs_shape, "<f4",
                                          self._t["obs"].device)
            self._obs_views = None

    def _stepped(self):
        """After a reset or a launch that stepped the envs (step, rollout, backtest): what was read of
        the state before is stale, and a sliding window has moved."""
        self._epoch += 1
        if self._obs_views is not None:
            self._follow_head()

    def _leave_sliding(self):
        """Back to a contiguous [N, W, F_obs] observation buffer for good: the current window is
        copied once and bound the classic way (a HIP graph reads `_t["obs"]` at capture time and
        RCCL sends a contiguous buffer: neither can follow a moving head)."""
        if self._obs_views is None:
            return
        torch = self._torch
        obs = self._t["obs"].contiguous()
        torch.cuda.synchronize(obs.device)
        b = _abi.GteOutputs()
        for k, t in self._t.items():
            setattr(b, k, (obs if k == "obs" else t).data_ptr())
        # the bind clears the two-slot terminal counter and rewinds it to slot 0: keep the last count readable
        _abi.check(self._lib, self._lib.gte_get_outputs(self._h, C.byref(self._out)))
        last = self._t["term_count"][int(self._out.term_slot)].clone()
        _abi.check(self._lib, self._lib.gte_bind_outputs(self._h, C.byref(b)))
        self._t["term_count"][0] = last
        self._t["obs"] = obs
        self._obs_slab = self._obs_views = None
        _abi.check(self._lib, self._lib.gte_get_outputs(self._h, C.byref(self._out)))

    # -- data movement helpers -------------------------------------------------------
    def _to_host(self, dev_ptr: int, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        _abi.check(self._lib, self._lib.gte_copy_to_host(self._h, C.c_void_p(dev_ptr),
                                                         out.ctypes.data, out.nbytes))
        return out

    def _read_snapshot(self, name: str, final: bool = False, tensor: bool = False):
        """One per-env array of the library's struct-of-arrays snapshot of the current state
        (`gte_get_state`) or of the terminal records (`gte_get_final_state`), taken once per
        step/reset on first use: a host copy, or (tensor) a torch view of it on the device."""
        dt = _abi.STATE_DTYPES[name]
        snap = self._snapshots[final]
        if snap[1] != self._epoch:
            get = self._lib.gte_get_final_state if final else self._lib.gte_get_state
            _abi.check(self._lib, get(self._h, C.byref(snap[0])))
            snap[1] = self._epoch
        if not tensor:
            return self._to_host(getattr(snap[0], name), _NP[dt], self.num_envs)
        t = self._snapshot_tensors.get((final, name))
        if t is None:
            t = _device_view(getattr(snap[0], name), (self.num_envs,), np.dtype(dt).str,
                             self._t["obs"].device)
            self._snapshot_tensors[(final, name)] = t
        return t

    def state(self, name: str) -> np.ndarray:
        """Host copy of one per-env state array (struct gte_state_view member)."""
        if self._snap_epoch == self._epoch and name in _abi.STATE_DTYPES:
            return np.ascontiguousarray(self._snap[name])  # numpy mode: fetched with the results
        return self._read_snapshot(name)

    def state_tensor(self, name: str):
        """One per-env state array as a torch tensor ON THE DEVICE, without a copy: a view of the
        library's struct-of-arrays snapshot (`gte_get_state`, refreshed once per step/reset on
        first use).  For device-side reward shaping / extra observation features:
        `envs.state_tensor("portfolio_valuation")`, `"real_position"`, `"idx"`, ...  The view is
        overwritten by the snapshot taken after a later step."""
        if self._torch is None:
            raise ValueError("state_tensor needs output='torch'")
        return self._read_snapshot(name, tensor=True)

    def read_output(self, name: str) -> np.ndarray:
        """Host copy of one output array of the last step/reset."""
        N = self.num_envs
        spec = {"obs": (np.float32, N * int(np.prod(self.obs_shape))),
                "final_obs": (np.float32, N * int(np.prod(self.obs_shape))),
                "reward": (np.float32, N), "reward64": (np.float64, N),
                "terminated": (np.uint8, N), "truncated": (np.uint8, N),
                "term_count": (np.int32, 2), "term_ids": (np.int32, N)}[name]
        if name == "obs" and self._obs_views is not None:  # a strided view: gte_read_obs packs it
            a = np.empty((N,) + self.obs_shape, np.float32)
            _abi.check(self._lib, self._lib.gte_read_obs(self._h, 0, N, a.ctypes.data))
            return a
        a = self._to_host(getattr(self._out, name), *spec)
        return a.reshape((N,) + self.obs_shape) if name in ("obs", "final_obs") else a

    def terminal_ids(self) -> np.ndarray:
        """Ids of the envs whose episode ended in the last step (sorted)."""
        _abi.check(self._lib, self._lib.gte_get_outputs(self._h, C.byref(self._out)))
        n = int(self.read_output("term_count")[self._out.term_slot])
        return np.sort(self.read_output("term_ids")[:n])

    def final_observations(self):
        """(env ids, terminal observations) of the envs that ended in the last step — the
        observation `TradingEnv.step` returned for them before the same-step reset
        (needs ``autoreset="same_step", final_obs=True``).  Torch mode: rows gathered on
        the device."""
        if not self.cfg.final_obs:
            raise ValueError("constructed without final_obs=True")
        ids = self.terminal_ids()
        if self.output == "torch":
            idx = self._torch.from_numpy(ids.astype(np.int64)).to(self._t["final_obs"].device)
            return ids, self._t["final_obs"][idx]
        return ids, self.read_output("final_obs")[ids]


    # -- vectorised access to what History logs (LazyInfo, BatchedHistory, metrics) ------------
    def _dataset_host_column(self, name):
        """One column of every dataset's info table (`data_<col>`, environments.py:142,260) or
        the index (`date`, :256), concatenated over the datasets: a (dataset, row) pair is ONE
        fancy index away, whatever N."""
        col = self._host_columns.get(name)
        if col is None:
            parts = []
            for ds in self.datasets:
                if name == "date":
                    parts.append(np.asarray(ds.index) if ds.index is not None else np.arange(ds.T))
                    continue
                c = name[len("data_"):]
                if ds.info_array is not None and c in ds.info_columns:
                    parts.append(ds.info_array[:, ds.info_columns.index(c)])
                elif c == "close":
                    parts.append(ds.close)
                else:
                    raise ValueError(f"Feature {name} does not exist ... Check the available "
                                     f"features : {self.info_keys}")
            col = np.concatenate(parts) if len(parts) > 1 else np.asarray(parts[0])
            if col.dtype == object:  # a numeric column staged through an object matrix
                try:
                    col = col.astype(np.float64)
                except (TypeError, ValueError):
                    pass
            self._host_columns[name] = col
        return col

    def _require_device_column(self, name):
        """Inside a graph capture: info column `name` must already be on the device (a host
        column cannot be read there, and its first upload is a copy a capture cannot hold)."""
        if self._dataset_host_column(name).dtype.kind not in "fiub":
            raise ValueError(f"History column {name!r} holds host values: it cannot be read inside a "
                             "graph capture")
        if name not in self._dev_columns:
            raise ValueError(f"History column {name!r} is uploaded to the device on first use, which "
                             "a graph capture cannot hold: read it once before capturing")

    def _dataset_column(self, name, ds, idx):
        """Values of info column `name` at (dataset, row) pairs; on the device for numeric
        columns in torch mode, else host arrays."""
        col = self._dataset_host_column(name)
        torch = self._torch
        if torch is not None and isinstance(ds, torch.Tensor):
            if col.dtype.kind in "fiub":
                dev = self._dev_columns.get(name)
                if dev is None:
                    dev = torch.as_tensor(col, device=ds.device)
                    self._dev_columns[name] = dev
                    self._dev_offsets = torch.as_tensor(self._ds_offsets, device=ds.device)
                return dev[self._dev_offsets[ds.long()] + idx.long()]
            ds, idx = ds.cpu().numpy(), idx.cpu().numpy()
        return col[self._ds_offsets[np.asarray(ds)] + np.asarray(idx)]

    def final_state(self, name: str) -> np.ndarray:
        """Host copy of one per-env array of the TERMINAL states (`gte_get_final_state`): row e
        is env e as it was when its last episode ended (same-step mode with final_obs)."""
        return self._read_snapshot(name, final=True)

    def _overlay(self, v, name, only=None):
        """`v` (a History column at the newest row, [N]) with the entries of the envs that ended
        in the last step replaced by their TERMINAL row's value (same-step mode, BatchedHistory
        terminal view); `only`: restrict to these envs."""
        torch = self._torch
        ended = self._t["terminated"] | self._t["truncated"]
        if only is not None:
            ended = ended & only
        # the terminal step's reward (the log row under it is a reset row: 0)
        t = history_column(name, lambda f: self._t["reward64"] if f == "reward" else
                           self._read_snapshot(f, final=True, tensor=True), self._pos_table, self)
        if not isinstance(t, torch.Tensor):  # host column (dates, objects)
            m = ended.cpu().numpy()
            out = np.array(v, copy=True)
            out[m] = np.asarray(t)[m]
            return out
        return torch.where(ended, t.to(v.dtype), v)

    def _final_entries(self) -> dict:
        """Gymnasium's `final_observation` / `final_info` (+ masks) for the envs that ended in
        the last step: the observation and the History row `TradingEnv.step` returned for them
        (environments.py:272) before the same-step reset."""
        N = self.num_envs
        ids, last = self.final_observations()
        mask = np.zeros(N, dtype=bool)
        mask[ids] = True
        f_obs = np.full(N, None, dtype=object)
        f_info = np.full(N, None, dtype=object)
        if len(ids):
            cols = {k: np.asarray(info_column(self, k, final=True))[ids] for k in self.info_keys}
            for j, e in enumerate(ids):
                f_obs[e] = last[j]
                f_info[e] = {k: v[j] for k, v in cols.items()}
        return {"final_observation": f_obs, "_final_observation": mask,
                "final_info": f_info, "_final_info": mask.copy()}

    # -- the device trajectory log ---------------------------------------------------------------
    def _log_view(self):
        _abi.check(self._lib, self._lib.gte_get_log(self._h, C.byref(self._logv)))
        return self._logv

    def _capturing(self) -> bool:
        """Is torch's current stream capturing a graph (StepGraph)?"""
        return self._torch is not None and self._torch.cuda.is_current_stream_capturing()

    def _log_order_on_device(self, view):
        """The physical log rows of the last L steps, oldest first, as a device tensor [L], computed
        from the log's row count on the device (gte_log_view.cursor) — in a graph, each replay's
        own rows.  Needs a full log."""
        torch = self._torch
        if self._log_cursor is None:
            self._log_cursor = _device_view(view.cursor, (2,), "<i8", self._t["obs"].device)
        slot, L = int(view.cursor_slot), int(view.L)
        count = self._log_cursor[slot:slot + 1]
        back = self._log_back if self._log_back is not None else torch.arange(-L, 0, device=count.device)
        return torch.remainder(back + count, L)

    def _device_result(self, x, what):
        """Inside a graph capture a callable's value must already be a device tensor."""
        if self._capturing():
            from .device_array import DeviceArray
            t = x.t if isinstance(x, DeviceArray) else x
            if not (isinstance(t, self._torch.Tensor) and t.is_cuda):
                raise ValueError(f"{what} returned {type(x).__name__} inside a graph capture: only "
                                 "device values (History columns and what is computed from them) "
                                 "can be captured")
        return x

    def _log_tensor(self, name):
        """torch view [L, N] of one log array (no copy)."""
        t = self._log_tensors.get(name)
        if t is None:
            v = self._log_view()
            # the log is one array of records [L, N]: a column is a strided view of it
            t = _device_view(getattr(v, name), (int(v.L), int(v.N)), np.dtype(_abi.LOG_DTYPES[name]).str,
                             self._t["obs"].device, (int(v.row_stride), int(v.env_stride)))
            self._log_tensors[name] = t
        return t

    def _log_rows(self, name, phys, order):
        """Log column `name`: physical row `phys` ([N]), per-env rows `phys[N]` ([N]), or — phys
        None — the rows `order`, oldest first ([R, N])."""
        N = self.num_envs
        if self._torch is not None:
            t = self._log_tensor(name)
            if phys is None:
                return t[self._torch.as_tensor(order, device=t.device)]
            if np.ndim(phys) == 0:
                return t[int(phys)]
            return t[phys.long(), self._torch.arange(N, device=t.device)]
        v, dt = self._log_view(), np.dtype(_abi.LOG_DTYPES[name])
        base, es, rs = int(getattr(v, name)), int(v.env_stride), int(v.row_stride)

        def rows_to_host(first, count):  # the records of `count` rows in one copy; the column = a strided view
            nbytes = (count - 1) * rs + (N - 1) * es + dt.itemsize
            raw = self._to_host(base + first * rs, np.dtype(np.uint8), nbytes)
            return np.ndarray(shape=(count, N), dtype=dt, buffer=raw, strides=(rs, es)).copy()
        if phys is not None and np.ndim(phys) == 0:
            return rows_to_host(int(phys), 1)[0]
        whole = rows_to_host(0, int(v.L))
        return whole[order] if phys is None else whole[np.asarray(phys), np.arange(N)]

    def _wrap(self, x):
        """What user callables receive: DeviceArray around device tensors, host arrays as is."""
        if self._torch is not None and isinstance(x, self._torch.Tensor):
            from .device_array import DeviceArray
            return DeviceArray(x)
        return x

    def _stack(self, cols):
        return self._torch.stack(cols, dim=-1) if self._torch is not None else np.stack(cols, axis=-1)

    def _arange_rows(self, n):
        if self._torch is not None:
            return self._torch.arange(n, device=self._t["obs"].device)
        return np.arange(n)

    def _set_log_reward(self, value):
        """`historical_info["reward", -1] = reward` (environments.py:267) for the batch."""
        if self._torch is not None:
            from .device_array import to_tensor
            value = self._device_result(value, "the value assigned to h['reward', -1]")
            r = to_tensor(value, self._t["obs"].device, self._torch.float64).contiguous()
            self._keep_reward = r
            _abi.check(self._lib, self._lib.gte_set_log_reward(self._h, C.c_void_p(r.data_ptr())))
        else:
            raise NotImplementedError("assigning log rewards needs output='torch'")

    def batched_history(self, terminal: bool = False):
        """The `BatchedHistory` of the batch right now (needs ``log_steps``): what custom reward /
        dynamic-feature / metric callables receive.  terminal=True: the same-step view in which
        envs that just ended show their terminal row as the newest one."""
        from .batched_history import BatchedHistory
        return BatchedHistory(self, terminal=terminal)

    def _apply_callables(self, after_reset: bool):
        """The user's own `reward_function` / `dynamic_feature_functions` (any callable that is
        not this package's default object), evaluated ONCE for the whole batch over a
        BatchedHistory, where the reference calls them per env: reward after `History.add`
        (environments.py:265-267: skipped — reward 0 — when done; rows a reset wrote have reward
        0, :196), then the dynamic features inside `_get_obs` (:153-154), which therefore see the
        reward.  Inside a graph capture nothing here waits for the device: the callables must
        return device values, and in same-step mode the fresh History is evaluated every step
        and merged with torch.where."""
        if self._reward_callable is None and not self._dyn_callables:
            return
        torch = self._torch
        if torch is None:
            raise NotImplementedError("custom callables in the batch need output='torch'")
        from .device_array import to_tensor
        dev = self._t["obs"].device
        N = self.num_envs
        same_step = self.cfg.autoreset == _abi.AUTORESET_SAME_STEP and not after_reset
        # same-step mode: an env that ended shows the callable its TERMINAL row (the log row of
        # this step already holds the state after the in-launch reset, which is what the NEXT
        # step's h[..., -2] must be)
        h = self.batched_history(terminal=same_step)
        ended = (self._t["terminated"] | self._t["truncated"]) if same_step else None
        capturing = self._capturing()
        if self._reward_callable is not None and not after_reset:
            r = to_tensor(self._device_result(self._reward_callable(h), "reward_function"), dev, torch.float64)
            if r.shape != (N,):
                raise ValueError(f"reward_function must return one value per env, got shape {tuple(r.shape)}")
            # one kernel applies the reference's rules (0 where terminated, :265, and on reset rows,
            # :196 — except, in same-step mode, under an ended env's terminal row) and writes the
            # f64 / f32 returns and the newest log row (:267)
            r = r.contiguous()
            self._keep_reward = r
            _abi.check(self._lib, self._lib.gte_apply_reward(self._h, C.c_void_p(r.data_ptr()),
                                                             1 if same_step else 0))
        if self._dyn_callables:
            cols = (C.c_void_p * self.cfg.n_dyn)()
            is_f64 = (C.c_int32 * self.cfg.n_dyn)()
            keep = []
            # (a capture cannot ask the device whether an env ended: it evaluates `fresh` every step)
            fresh = self.batched_history() if (same_step and (capturing or bool(ended.any()))) else None
            for i, fn in self._dyn_callables:
                v = to_tensor(self._device_result(fn(h), "a dynamic feature function"), dev, None)
                if v.dtype not in (torch.float32, torch.float64):
                    v = v.to(torch.float64)
                if v.shape != (N,):
                    v = v.expand(N) if v.dim() == 0 else v.reshape(N)
                if fresh is not None:
                    # the terminal observation shows the feature of the terminal row, the returned
                    # observation the one of the reset row (reset() evaluates it on a 1-row History)
                    col = self.datasets[0].n_static + i
                    fo = self._t["final_obs"]
                    if capturing:  # (a boolean-mask write waits for the device)
                        last = fo[:, -1, col] if fo.dim() == 3 else fo[:, col]
                        last.copy_(torch.where(ended, v.to(fo.dtype), last))
                    elif fo.dim() == 3:
                        fo[ended, -1, col] = v[ended].to(fo.dtype)
                    else:  # windows=None: the observation is one row
                        fo[ended, col] = v[ended].to(fo.dtype)
                    v_fresh = self._device_result(fn(fresh), "a dynamic feature function")
                    v = torch.where(ended, to_tensor(v_fresh, dev, v.dtype), v)
                v = v.contiguous()
                keep.append(v)
                cols[i] = v.data_ptr()
                is_f64[i] = 1 if v.dtype == torch.float64 else 0
            self._keep_dyn = keep  # alive until the (stream-ordered) kernel has read them
            _abi.check(self._lib, self._lib.gte_set_dynamic_columns(self._h, cols, is_f64))

    # -- trajectory log ------------------------------------------------------------------
    def add_metric(self, name, function):
        """`TradingEnv.add_metric` (environments.py:274-278): `function(history)` is evaluated
        for every finished env by :meth:`episode_metrics` (needs ``log_steps``)."""
        if not self.cfg.log_steps:
            raise ValueError("add_metric needs log_steps > 0 (the History comes from the device log)")
        self.log_metrics.append({"name": name, "function": function})

    def read_log_envs(self, env_ids, finished: bool = False, max_rows=None) -> dict:
        """The logged episode of each listed env in ONE device->host transfer
        (`gte_read_log_envs`): dict of arrays [n_ids, max_rows] — the log columns of
        `_abi.LOG_DTYPES` — plus "n_rows" [n_ids]; rows 0 .. n_rows[j]-1 of env j are valid,
        oldest first.  Views of the library's pinned staging buffer: valid until the next call.
        finished=True: the episodes that just ENDED (same-step auto-reset with ``final_obs``)."""
        L = int(self.cfg.log_steps)
        if not L:
            raise ValueError("constructed with log_steps=0")
        ids = np.ascontiguousarray(np.asarray(env_ids, dtype=np.int32).reshape(-1))
        b = _abi.GteLogBatch()
        _abi.check(self._lib, self._lib.gte_read_log_envs(
            self._h, ids.ctypes.data, len(ids), int(max_rows or 0), 1 if finished else 0, C.byref(b)))
        n, R = int(b.n_ids), int(b.max_rows)
        out = {"n_rows": np.zeros(0, np.int32)}
        if n:
            out["n_rows"] = np.frombuffer((C.c_int32 * n).from_address(b.n_rows), dtype=np.int32)
        for name, dt in _abi.LOG_DTYPES.items():
            dt = np.dtype(dt)
            if not n:
                out[name] = np.zeros((0, R), dt)
                continue
            raw = (C.c_char * (n * R * dt.itemsize)).from_address(getattr(b, name))
            out[name] = np.frombuffer(raw, dtype=dt).reshape(n, R)
        return out

    def histories(self, env_ids, finished: bool = False) -> list:
        """One `History` per listed env: its current (or, finished=True, just finished) episode
        with the reference's columns (environments.py:186-197, 253-264), rebuilt from the device
        trajectory log.  ONE transfer for all of them; the columns are built once over the
        concatenated rows and cut per env."""
        from .history import ColumnBlock, History
        ids = np.asarray(env_ids, dtype=np.int64).reshape(-1)
        if finished and not self.cfg.final_obs:
            raise ValueError("history(finished=True) needs autoreset='same_step', final_obs=True")
        b = self.read_log_envs(ids, finished=finished)
        n = b["n_rows"].astype(np.int64)
        if finished and len(ids):
            last = b["flags"][np.arange(len(ids)), np.maximum(n - 1, 0)]
            bad = np.nonzero((n == 0) | ((last & 3) == 0))[0]
            if len(bad):
                raise ValueError(f"env {int(ids[bad[0]])} did not end in the last step")
        R = b["idx"].shape[1]
        valid = np.arange(R)[None, :] < n[:, None]
        # the valid rows of every env, env after env, copied out of the staging buffer now (the next
        # read rewrites it): one boolean-mask copy per raw column, 12 small arrays
        flat = {name: b[name][valid] for name in _abi.LOG_DTYPES}
        pos_table = np.empty(len(self.positions), dtype=object)
        pos_table[:] = self.positions
        # Every column is built on first use, over all the episodes at once, and cut per env: a
        # metric that reads `h["position"]` never pays for dates or portfolio distributions.
        block = ColumnBlock({c: (lambda c=c: history_column(c, flat.__getitem__, pos_table, self))
                             for c in history_columns(self)})
        ends = np.cumsum(n).tolist()
        out, lo = [], 0
        for hi in ends:
            out.append(History.from_block(block, lo, hi))
            lo = hi
        return out

    def history(self, env_id: int, finished: bool = False):
        """The current (or just finished) episode of one env as a `History` with the
        reference's columns (environments.py:186-197, 253-264: idx, step, date, position_index,
        position, real_position, data_*, portfolio_valuation, portfolio_distribution_*, reward),
        rebuilt from the device trajectory log.  Episodes longer than ``log_steps`` are
        truncated at the front.  With auto-reset disabled, a frozen env (ended on its dataset's
        last row) logs a copy of its last row every step until it is reset: the History leaves
        the copies out, but they take log rows too, so the frozen time counts towards the
        ``log_steps`` rows kept (once only copies are left, one row with reward 0 remains).

        finished=True (same-step auto-reset with ``final_obs``, right after the step in which the
        env ended): the episode that just FINISHED — its rows from the log plus the terminal row
        from the env's terminal record (that step's log row already describes the new episode).
        For many envs use :meth:`histories` (one transfer for all of them)."""
        return self.histories([int(env_id)], finished=finished)[0]

    def save_for_render(self, env_id: int, dir="render_logs"):
        """`TradingEnv.save_for_render` (environments.py:296-307) for one env of the batch: the
        dataset's frame joined with the episode History rebuilt from the device trajectory log
        (needs ``log_steps``), pickled as `<name>_<timestamp>.pkl` for the reference's renderer.
        -> path of the file."""
        import datetime
        import os
        import pandas as pd
        h = self.history(env_id)
        ds = self.datasets[int(self.state("dataset_index")[env_id])]
        missing = [c for c in ("open", "high", "low", "close") if c not in (ds.info_columns or [])]
        assert not missing, (
            "Your DataFrame needs to contain columns : open, high, low, close to render !")
        frame = pd.DataFrame(ds.info_array, columns=ds.info_columns, index=ds.index)
        logged = pd.DataFrame({c: h[c] for c in h.columns}).set_index("date").sort_index()
        os.makedirs(dir, exist_ok=True)
        stamp = datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
        path = os.path.join(dir, f"{ds.name}_env{int(env_id)}_{stamp}.pkl")
        frame.join(logged, how="inner").to_pickle(path)
        return path

    def episode_metrics(self, env_ids=None) -> dict:
        """Episode-end metrics of `calculate_metrics` (environments.py:279-286) for the envs
        whose episode just ended (default: `terminal_ids()`), from the device state:
        "Market Return" = close[idx] / close[start_idx] - 1 and "Portfolio Return" =
        portfolio_valuation / initial value - 1, as float arrays plus the reference's
        formatted strings.  Call it right after the terminal step (with next-step auto-reset
        the state still belongs to the finished episode until the following step; with
        same-step auto-reset and ``final_obs`` the terminal records are used)."""
        ids = self.terminal_ids() if env_ids is None else np.asarray(env_ids, dtype=np.int64)
        state = self.final_state if (self.cfg.final_obs and env_ids is None) else self.state
        use_final = bool(self.cfg.final_obs and env_ids is None)
        ds, idx, start = (state(k)[ids] for k in ("dataset_index", "idx", "start_idx"))
        pv = state("portfolio_valuation")[ids]
        close_now = np.asarray(self._dataset_column("data_close", ds, idx), dtype=np.float64)
        close_0 = np.asarray(self._dataset_column("data_close", ds, start), dtype=np.float64)
        market = close_now / close_0 - 1 if len(ids) else np.zeros(0)
        portfolio = pv / self.cfg.portfolio_initial_value - 1
        out = {"env_ids": ids, "market_return": market, "portfolio_return": portfolio,
               "episode_length": state("step")[ids] + 1,
               "Market Return": [f"{100 * m:5.2f}%" for m in market.tolist()],
               "Portfolio Return": [f"{100 * r:5.2f}%" for r in portfolio.tolist()]}
        if self.log_metrics:  # custom metrics over each finished env's History (:285-286)
            hists = self.histories(ids, finished=use_final)  # ONE transfer for all of them
            for metric in self.log_metrics:
                out[metric["name"]] = [metric["function"](h) for h in hists]
        return out

    def _rotate_returns(self):
        """Point the next step at the next packed return buffer (gte_bind_returns)."""
        self._ret_slot = (self._ret_slot + 1) % self.return_slots
        buf, views, ptrs = self._slot_views[self._ret_slot]
        _abi.check(self._lib, self._lib.gte_bind_returns(self._h, *ptrs))
        self.packed_returns = buf
        self._out.reward, self._out.terminated, self._out.truncated = (p.value for p in ptrs)
        t = self._t
        t["reward"], t["terminated"], t["truncated"] = views

    @property
    def return_slot(self) -> int:
        """Row of the [return_slots, 6N] buffer the NEXT step writes its returns into."""
        return (self._ret_slot + 1) % self.return_slots

    def return_block(self, first: int, count: int):
        """uint8 [count, 6N]: the packed returns in rows first..first+count-1 (contiguous)."""
        if not (0 <= first and first + count <= self.return_slots):
            raise IndexError("return block out of range")
        return self._packed_all[first:first + count]

    def _results(self):
        if self.output == "torch":
            t = self._t
            return t["obs"], t["reward"], t["terminated"], t["truncated"]
        # host arrays: state, returns and observations of the whole batch in ONE transfer
        self._snap, self._snap_obs = self.read_envs(view=not self.copy)
        self._snap_epoch = self._epoch
        snap = self._snap
        return (self._snap_obs, np.ascontiguousarray(snap["reward"]),
                snap["terminated"].astype(bool), snap["truncated"].astype(bool))

    # -- the Env API -------------------------------------------------------------------
    def reset(self, seed=None, options=None, *, mask=None, inject_idx=None,
              inject_position_index=None, inject_dataset=None):
        """`TradingEnv.reset` (environments.py:163-199) for all envs, or those in `mask`.

        `seed` is accepted for API compatibility; like in the reference (whose reset
        draws from the global NumPy RNG) it does not reseed the episode draws — the
        device Philox stream is keyed by the constructor's `seed`."""
        def arr(a, dt):
            if a is None:
                return None, None
            a = np.ascontiguousarray(np.asarray(a, dtype=dt))
            if a.shape != (self.num_envs,):
                raise ValueError(f"expected shape ({self.num_envs},), got {a.shape}")
            return a, a.ctypes.data
        m, mp = arr(mask, np.uint8)
        a, ap = arr(inject_idx, np.int32)
        b, bp = arr(inject_position_index, np.int32)
        c, cp = arr(inject_dataset, np.int32)
        _abi.check(self._lib, self._lib.gte_reset(self._h, mp, ap, bp, cp))
        self._was_reset = True
        self._stepped()
        self._apply_callables(after_reset=True)
        return self._results()[0], LazyInfo(self)

    def set_autoreset_injection(self, idx=None, position_index=None, dataset=None):
        """Queue the draws of later auto-resets: i32 [N, n_episodes] arrays (parity runs)."""
        arrs = [np.asarray(x) for x in (idx, position_index, dataset) if x is not None]
        n = 0 if not arrs else arrs[0].reshape(self.num_envs, -1).shape[1]
        def arr(a):
            if a is None:
                return None, None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(self.num_envs, n))
            return a, a.ctypes.data
        a, ap = arr(idx)
        b, bp = arr(position_index)
        c, cp = arr(dataset)
        _abi.check(self._lib, self._lib.gte_set_autoreset_injection(self._h, n, ap, bp, cp))

    def add_limit_order(self, position_index, limit, persistent=False):
        """`TradingEnv.add_limit_order` (environments.py:227-231) for a batch.

        position_index: i32 [N] index into `positions` of each env's order target, -1 for
        "no order for this env"; limit: f64 [N]; persistent: bool or bool [N]."""
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(position_index, np.int32), (self.num_envs,)))
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, np.float64), (self.num_envs,)))
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(persistent, np.uint8), (self.num_envs,)))
        _abi.check(self._lib, self._lib.gte_add_limit_orders(self._h, a.ctypes.data, b.ctypes.data,
                                                             c.ctypes.data))
        self._epoch += 1

    def step(self, actions):
        """`TradingEnv.step` (environments.py:233-272) for every env in one launch.

        actions: position indices, shape (N,); -1 (or None entries) = hold (:234).
        A torch int32 CUDA tensor is used in place; anything else goes through a
        host->device copy."""
        self._launch_step(actions)
        self._apply_callables(after_reset=False)
        if self.verbose > 0 and self._user_log and not self._capturing():  # (a report synchronises)
            import time
            now = time.monotonic()
            if now - self._last_report >= self.verbose_interval:
                self._last_report = now
                self.log()
        obs, reward, term, trunc = self._results()
        return obs, reward, term, trunc, LazyInfo(self)

    def log(self):
        """`TradingEnv.log` after `calculate_metrics` (environments.py:269-271, :279-294) for the
        envs whose episode ended in the last step: one line each, the reference's text —
        "Market Return : ..   |   Portfolio Return : ..   |   " plus every `add_metric` entry.  A
        batch can end hundreds of episodes per step, so at most `verbose_max_lines` lines are
        printed, then a count.  Costs a device synchronisation, which is why `step()` only does it
        when the user asked for a trajectory log (``log_steps`` > 0: an env set up for metrics, not
        the bare hot path, and not the 2-row log a Python callable brings with it), `verbose` > 0,
        and at most once per `verbose_interval` seconds (episodes that end between two reports
        are not listed; `episode_metrics()` after any step gives them all).  In same-step mode it needs ``final_obs`` (the terminal
        records); without them the finished episodes' final state is gone and nothing is printed."""
        if self.verbose <= 0:
            return
        if self.cfg.autoreset == _abi.AUTORESET_SAME_STEP and not self.cfg.final_obs:
            return
        m = self.episode_metrics()
        n = len(m["env_ids"])
        names = ["Market Return", "Portfolio Return"] + [x["name"] for x in self.log_metrics]
        for j in range(min(n, self.verbose_max_lines)):
            print("".join(f"{k} : {m[k][j]}   |   " for k in names))
        if n > self.verbose_max_lines:
            print(f"... and {n - self.verbose_max_lines} more episodes ended in this step")

    def _launch_step(self, actions):
        """The launch half of step(): nothing is copied back."""
        torch = self._torch
        on_device = torch is not None and isinstance(actions, torch.Tensor) and actions.is_cuda
        if on_device:
            if actions.dtype != torch.int32 or not actions.is_contiguous():
                actions = actions.to(torch.int32).contiguous()
            if actions.shape != (self.num_envs,):
                raise ValueError(f"expected {self.num_envs} actions")
        else:
            if torch is not None and isinstance(actions, torch.Tensor):
                actions = actions.cpu().numpy()
            a = np.array([-1 if x is None else x for x in actions], dtype=np.int32) \
                if isinstance(actions, (list, tuple)) else np.asarray(actions, dtype=np.int32)
            a = np.ascontiguousarray(a)
            if a.shape != (self.num_envs,):
                raise ValueError(f"expected {self.num_envs} actions")
            if a.size and (a.max() >= len(self.positions) or a.min() < -1):
                raise IndexError("list index out of range")  # positions[position_index] (:234)
        # whichever way the actions arrive, the step writes the NEXT row of the return buffers
        if self.return_slots > 1:
            self._rotate_returns()
        if on_device:
            self._keep = actions  # keep alive until the launch has consumed it
            _abi.check(self._lib, self._lib.gte_step(self._h, C.c_void_p(actions.data_ptr()), 1))
        else:
            _abi.check(self._lib, self._lib.gte_step(self._h, a.ctypes.data, 0))
        self._stepped()

    def capture_steps(self, body, n_steps: int):
        """Record `body(i)` for i in range(n_steps) — each call taking ONE `step()` with a CUDA
        int32 action tensor, plus any torch code around it (the policy) — into a HIP graph
        (`torch.cuda.graph`); `.replay()` on the returned `StepGraph` runs them again with one
        host call.  For launch-bound batches (config 2: 4 096 envs).  n_steps must be even.

        Logged envs and Python callables are captured too, once the log is full (``log_steps``
        eager steps, the reset included): the History reads of the callables pick their rows on
        the device, the callables must return device values, and same-step terminal observations
        are merged with torch.where.  Inside the capture `verbose` reports are skipped (a report
        synchronises); `return_slots` > 1 is refused.  See step_graph.py."""
        from .step_graph import StepGraph
        self._leave_sliding()  # (the captured body reads _t["obs"]: one buffer for every replay)
        return StepGraph(self, body, n_steps)

    def read_envs(self, first: int = 0, count=None, with_obs: bool = True, view: bool = False):
        """(snapshots, obs): a structured array [count] with the fields of struct
        gte_env_snapshot (state, reward f64, terminated, truncated) and the observations
        [count, *obs_shape] (or None) of envs first..first+count-1, fetched with one
        device->host transfer (`gte_read_envs`).  view=True: arrays over the library's pinned
        staging buffer, valid until the next read (`gte_read_envs_view`)."""
        count = self.num_envs - first if count is None else int(count)
        if view:
            ps, po = C.c_void_p(), C.c_void_p()
            _abi.check(self._lib, self._lib.gte_read_envs_view(
                self._h, int(first), count, 1 if with_obs else 0, C.byref(ps), C.byref(po)))
            snap = np.frombuffer((C.c_char * (96 * count)).from_address(ps.value),
                                 dtype=_abi.SNAPSHOT_DTYPE)
            obs = None
            if with_obs:
                n = count * int(np.prod(self.obs_shape))
                obs = np.frombuffer((C.c_float * n).from_address(po.value), dtype=np.float32
                                    ).reshape((count,) + self.obs_shape)
            return snap, obs
        snap = np.empty(count, dtype=_abi.SNAPSHOT_DTYPE)
        obs = np.empty((count,) + self.obs_shape, np.float32) if with_obs else None
        _abi.check(self._lib, self._lib.gte_read_envs(
            self._h, int(first), count, snap.ctypes.data, obs.ctypes.data if with_obs else None))
        return snap, obs

    def read_env(self, env_index: int = 0, with_obs: bool = True):
        """(GteEnvSnapshot, obs ndarray | None) of ONE env after the last step/reset: state,
        returns and observation in a single device->host transfer (`gte_read_env`)."""
        snap = _abi.GteEnvSnapshot()
        obs = np.empty(self.obs_shape, np.float32) if with_obs else None
        _abi.check(self._lib, self._lib.gte_read_env(
            self._h, int(env_index), C.byref(snap), obs.ctypes.data if with_obs else None))
        return snap, obs

    def _sequence_actions(self, actions, what):
        """The [K, N] action sequence of rollout() / backtest() as a contiguous int32 device tensor
        (None = hold, like step()); refuses what a launch of K steps cannot serve."""
        torch = self._torch
        if torch is None:
            raise ValueError(f"{what} needs output='torch'")
        if self._reward_callable is not None or self._dyn_callables:
            raise NotImplementedError(f"a fused {what} runs all steps on the device: custom Python "
                                      "reward / dynamic-feature callables need step()")
        dev = self._t["obs"].device
        if not (isinstance(actions, torch.Tensor) and actions.is_cuda):
            a = np.asarray([[-1 if x is None else x for x in row] for row in actions]
                           if isinstance(actions, (list, tuple)) else actions, dtype=np.int32)
            if a.size and (a.max() >= len(self.positions) or a.min() < -1):
                raise IndexError("list index out of range")
            actions = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        actions = actions.to(torch.int32).contiguous()
        if actions.dim() != 2 or actions.shape[1] != self.num_envs or actions.shape[0] < 1:
            raise ValueError(f"expected actions of shape (K, {self.num_envs})")
        return actions

    def rollout(self, actions, *, keep_obs=False, valuation=False, reward64=False, out=None):
        """K consecutive step() calls for action sequences known in advance, in ONE launch
        (`gte_rollout`: backtests of precomputed strategies, random-policy collection).

        actions: int32 [K, N] (-1 = hold), a torch CUDA tensor or anything array-like.
        Returns a dict of device tensors: reward f32 [K, N], terminated / truncated bool
        [K, N], obs — [K, N, *obs_shape] with keep_obs=True, else the observation after the
        last step [N, *obs_shape] —, and on request valuation f64 [K, N] (portfolio value
        after each step) and reward64.  State and results equal K single steps exactly.
        out: the dict a previous call with the same K and options returned — its tensors are
        written again instead of allocating new ones (K x 168 MB of observations at the headline
        shape; where a buffer lands in memory also moves the store rate by a few percent)."""
        torch = self._torch
        actions = self._sequence_actions(actions, "rollout")
        dev = self._t["obs"].device
        K, N = int(actions.shape[0]), self.num_envs
        want = {"reward": ((K, N), torch.float32), "terminated": ((K, N), torch.bool),
                "truncated": ((K, N), torch.bool)}
        if keep_obs:
            want["obs"] = ((K, N) + self.obs_shape, torch.float32)
        if valuation:
            want["valuation"] = ((K, N), torch.float64)
        if reward64:
            want["reward64"] = ((K, N), torch.float64)
        if out is not None:
            out = {k: out[k] for k in want}  # KeyError: not the result of a matching call
            for k, (shape, dt) in want.items():
                t = out[k]
                if tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"out[{k!r}] does not match this rollout")
        else:
            with torch.cuda.device(dev):
                out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in want.items()}
        b = _abi.GteRolloutBufs()
        for k, t in out.items():
            setattr(b, k, t.data_ptr())
        self._keep = (actions, out)  # alive until the launch has consumed them
        _abi.check(self._lib, self._lib.gte_rollout(self._h, C.c_void_p(actions.data_ptr()), K,
                                                    C.byref(b)))
        self._stepped()
        if not keep_obs:
            out["obs"] = self._t["obs"]
        return out

    def backtest(self, actions, *, resume=False):
        """K consecutive step() calls like `rollout(actions)` that keep, instead of per-step rows,
        one record of running statistics per env (`gte_backtest`): transitions, reward sum and sum
        of squares, peak and maximum drawdown, trades, finished episodes and their returns.
        The statistics are reduced where the state lives, in registers, so a backtest costs one
        store per env and call whatever its length, and it can be fed in chunks of actions:

            stats = env.backtest(actions[:4096])
            stats = env.backtest(actions[4096:], resume=True)

        resume=False clears the records first (they then start from the env's current state);
        resume=True continues them — an env that was `reset()` in between restarts its peak and
        its position for the trade count and keeps its sums.  State, return buffers, terminal
        list and observation afterwards are those of K single steps.  Returns a `BacktestStats`."""
        from .backtest_stats import BacktestStats
        actions = self._sequence_actions(actions, "backtest")
        ptr = C.c_void_p()
        self._keep = (actions,)  # alive until the launch has consumed them
        _abi.check(self._lib, self._lib.gte_backtest(self._h, C.c_void_p(actions.data_ptr()),
                                                     int(actions.shape[0]), 0 if resume else 1, C.byref(ptr)))
        self._stepped()
        self._backtest_map = None  # (no strategies: by_strategy() needs its arguments)
        return BacktestStats(self, ptr.value)

    def track_trades(self, on=True, list_capacity=0):
        """Keep round-trip TRADE statistics next to the backtest statistics (`gte_track_trades`): while on,
        `backtest()` and `backtest_signals()` maintain a second 128-byte record per env — closed trades, wins and
        losses, gross profit and loss, best and worst trade, holding times, time in the market, losing streaks
        (the rule is stated in include/gte.h) — reduced in registers while they step, and the `BacktestStats`
        they return has them as `.trade_stats`.  Off (the default) every call launches exactly the kernels it
        launches without this feature.  `list_capacity` > 0 (`gte_track_trade_list`) also keeps a PER-TRADE LIST:
        the first `list_capacity` closed trades of every env since the records were cleared — entry and exit row,
        the two valuations, the position, the holding time and how it ended — written where the trade closes and
        read with `stats.trade_stats.trades()`; 0 turns the list off, and so does ``track_trades(False)``.  The
        first backtest call after a change — on, off, another capacity — clears the records whatever its
        `resume` says.  Needs a `reset()` before it; waits for the env's stream."""
        if isinstance(list_capacity, bool) or int(list_capacity) != list_capacity:
            raise TypeError("list_capacity must be an integer")
        ptr = C.c_void_p()
        _abi.check(self._lib, self._lib.gte_track_trades(self._h, 1 if on else 0, C.byref(ptr)))
        self._trades_ptr = int(ptr.value or 0) if on else 0
        if not on:
            self._trade_list_capacity = 0  # (switching tracking off turned the list off)
        elif self._trade_list_capacity or int(list_capacity):
            _abi.check(self._lib, self._lib.gte_track_trade_list(self._h, int(list_capacity), None))
            self._trade_list_capacity = int(list_capacity)

    def track_periods(self, period_of_row, n_periods=None):
        """Keep PERIOD statistics next to the backtest statistics (`gte_bind_periods`, `gte_track_periods`):
        ``period_of_row[t]`` is the period id of market row t — a calendar month, a walk-forward fold, train /
        embargo / test (`gym_trading_env_amd.periods` makes such rows) — as one integer array [T], or a list of
        them, one per dataset.  While on, `backtest()` and `backtest_signals()` maintain one 32-byte record per
        (env, period): reward sum, sum of squares, transitions, position changes and episodes of the transitions
        whose row lay in that period (a row with an id outside [0, n_periods), such as -1, counts nowhere; the
        rule is stated in include/gte.h), reduced in registers while they step, and the `BacktestStats` they
        return has them as `.period_stats`.  `n_periods` defaults to the largest id + 1; at most 128.
        ``track_periods(None)`` turns tracking off: then every call launches exactly the kernels it launches
        without this feature.  The first backtest call after a change clears the records whatever its `resume`
        says.  Not together with `track_trades()`.  Needs a `reset()` before it; waits for the env's stream.
        Another `n_periods` allocates new records and frees the old ones: a `PeriodStats` from before then
        raises instead of reading them (clone the fields, or take `.numpy()`, of a result that is to be compared
        with a run under another period count).  If binding a row fails, tracking is left off."""
        ptr = C.c_void_p()
        if period_of_row is None:
            _abi.check(self._lib, self._lib.gte_track_periods(self._h, 0, C.byref(ptr)))
            self._periods = None
            return
        D = len(self.datasets)
        rows = list(period_of_row) if isinstance(period_of_row, (list, tuple)) and len(period_of_row) and \
            np.ndim(period_of_row[0]) == 1 else [period_of_row] * D
        if len(rows) != D:
            raise ValueError(f"{len(rows)} period rows for {D} datasets")
        staged = []
        for d, row in enumerate(rows):
            a = np.asarray(row.cpu() if hasattr(row, "cpu") else row)
            if a.ndim != 1 or a.shape[0] != self.datasets[d].T:
                raise ValueError(f"period_of_row of dataset {d}: shape {a.shape}, the dataset has {self.datasets[d].T} rows")
            if a.dtype.kind not in "iu":
                raise TypeError("period_of_row must hold integers")
            if a.size and (a.min() < -128 or a.max() > 127):
                raise ValueError("period ids must fit int8 (ids outside [0, n_periods) count nowhere)")
            staged.append(np.ascontiguousarray(a, dtype=np.int8))
        if n_periods is None:
            n_periods = max(int(a.max()) for a in staged) + 1
        if isinstance(n_periods, bool) or int(n_periods) != n_periods or not 1 <= int(n_periods) <= _abi.GTE_MAX_PERIODS:
            raise ValueError(f"n_periods must lie in [1, {_abi.GTE_MAX_PERIODS}]")
        # switch first: a refusal (no reset yet, trade tracking on, a capture) leaves the rows as they were
        _abi.check(self._lib, self._lib.gte_track_periods(self._h, int(n_periods), C.byref(ptr)))
        records = (int(ptr.value or 0), int(n_periods))
        if records != self._period_records:  # another B: the library freed the records older results view
            self._period_records = records
            self._period_generation += 1
        try:
            for d, a in enumerate(staged):
                _abi.check(self._lib, self._lib.gte_bind_periods(self._h, d, a.ctypes.data))
        except Exception:
            # a bind that fails partway would leave tracking on with some datasets on their old row or on none
            self._periods = None
            self._lib.gte_track_periods(self._h, 0, None)
            raise
        self._periods = records + (self._period_generation,)

    # -- signal tables: the action looked up on the device by the row an env stands on -----
    def bind_signals(self, signals, dataset=None):
        """Bind per-strategy signal tables (`gte_bind_signals`): ``signals[s][t]`` is the position
        index strategy ``s`` wants while an env stands on row ``t`` — the action of the step it
        takes from there, ``env.step(a if 0 <= a < len(positions) else None)``.  Any value outside
        ``[0, len(positions))`` means hold.

        signals: integers that fit int8, shape [S, T] — a torch CUDA tensor or anything array-like —
        for dataset `dataset` (default: the only one), or with ``dataset=None`` a list of D such
        tables, one per resident dataset, all with the same S.  Each table is copied once into an
        int8 device tensor whose rows are padded to a multiple of 16 bytes, which the env keeps
        alive.  A table whose T is not its dataset's, or whose S differs from the tables already
        bound, is refused.  ``signals=None`` unbinds.  Uploading a dataset again unbinds its table."""
        torch = self._torch
        if torch is None:
            raise ValueError("bind_signals needs output='torch'")
        D = len(self.datasets)
        if dataset is None:
            if signals is None:
                tables = {d: None for d in range(D)}
            elif isinstance(signals, (list, tuple)) and len(signals) == D and \
                    all(getattr(t, "ndim", None) == 2 or (isinstance(t, (list, tuple)) and t and
                                                         isinstance(t[0], (list, tuple))) for t in signals):
                tables = dict(enumerate(signals))
            elif D == 1:
                tables = {0: signals}
            else:
                raise ValueError(f"expected a list of {D} signal tables, one per dataset (or dataset=d)")
        else:
            if not 0 <= int(dataset) < D:
                raise IndexError(f"dataset {dataset} out of range")
            tables = {int(dataset): signals}
        from . import signals as sig
        dev = self._t["obs"].device
        padded = {}
        for d, t in tables.items():
            if t is None:
                continue
            if isinstance(t, torch.Tensor) and t.is_cuda:
                if t.dim() != 2 or t.is_floating_point() or t.is_complex():
                    raise TypeError("a signal table is a two-dimensional integer tensor")
                if t.dtype != torch.int8 and t.numel() and (int(t.min()) < -128 or int(t.max()) > 127):
                    raise ValueError("signal table values must fit int8")
                S, T = int(t.shape[0]), int(t.shape[1])
                with torch.cuda.device(dev):
                    buf = torch.full((S, sig.row_stride(T)), -1, dtype=torch.int8, device=dev)
                buf[:, :T] = t.to(device=dev, dtype=torch.int8)
            else:
                host = sig.as_int8_table(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
                S, T = host.shape
                buf = torch.from_numpy(sig.pad_rows(host)).to(dev)
            if T != self.datasets[d].T:
                raise ValueError(f"signal table of dataset {d} has {T} columns, the dataset {self.datasets[d].T} rows")
            padded[d] = buf
        self._check_one_s(padded, tables)
        if padded:
            torch.cuda.current_stream(dev).synchronize()  # the copies above: the env may launch on another stream
        for d, t in tables.items():
            if t is None:
                _abi.check(self._lib, self._lib.gte_bind_signals(self._h, d, None, 0, 0))
                self._signals.pop(d, None)
            else:
                self._bind_padded(d, padded[d])

    def _check_one_s(self, padded, replaced):
        """one S: over the padded tables of this call and those that stay bound"""
        kept = {d: t for d, t in self._signals.items() if d not in replaced}
        sizes = {int(t.shape[0]) for t in list(padded.values()) + list(kept.values())}
        if len(sizes) > 1:
            raise ValueError(f"signal tables must have one number of strategies, got {sorted(sizes)}")

    def _bind_padded(self, d, buf):
        """Bind the padded int8 [S, stride] device tensor `buf`, complete on the env's stream, to
        dataset d and keep it alive (the bind step of bind_signals and build_signals)."""
        from . import signals as sig
        assert buf.data_ptr() % sig.PIECE == 0 and buf.is_contiguous()
        _abi.check(self._lib, self._lib.gte_bind_signals(self._h, d, C.c_void_p(buf.data_ptr()),
                                                         int(buf.shape[0]), int(buf.shape[1])))
        self._signals[d] = buf

    def build_signals(self, indicators, rules, dataset=None, bind=True):
        """Build signal tables ON THE DEVICE from indicator rules (`gte_build_signals`): one rule per
        strategy (`signals.rules`, `signals.RULE_DTYPE`; the rule is stated in include/gte.h) over a
        bank of indicators f32 [C, T] of the dataset (`signals.sma_bank`, feature columns, anything).
        Returns the table as a torch int8 [S, T] view of a padded device tensor — complete for torch
        to read when the call returns — and, with ``bind=True``, binds that same tensor as
        `bind_signals` would, without a second copy.  No [S, T] array exists on the host.

        indicators: a NumPy array or a CUDA f32 tensor [C, T] for dataset `dataset` (default: the
        only one); with ``dataset=None`` and D > 1 a list of D banks, one per resident dataset, and
        the result is a list of D tables.  A CUDA bank whose rows are 16-byte aligned and padded to
        `signals.bank_stride(T)` floats (a ``[:, :T]`` view of such a tensor) is read in place.
        rules: a `RULE_DTYPE` array [S], whose `a` / `b` are checked against the bank here, or a
        CUDA tensor uint8 [S, 32] / int32 [S, 8] of the same bytes, which is the caller's contract:
        the kernel gives a rule that names no indicator a row of -1.  One rule array serves every
        dataset.  The caller's rule order is kept (a row index is a strategy id).  One wavefront
        builds one row, and the waves that run together share the bank through L2: rules sorted by
        ``(a, b)`` built 65 536 rows x 33 259 columns over 256 indicators 36 % faster than the same
        rules in random order (16 % at 4 096 rows; DESIGN.md §4, `tools/signal_build_bench.py`), so
        sort a large sweep by indicator before it becomes the strategy numbering."""
        torch = self._torch
        if torch is None:
            raise ValueError("build_signals needs output='torch'")
        from . import signal_device as sd, signals as sig
        dev = self._t["obs"].device
        banks, wants_list = sd.per_dataset(indicators, len(self.datasets), dataset, "indicator banks")
        d_rules, host_rules = sd.records(rules, sig.RULE_DTYPE, "RULE_DTYPE", ((torch.uint8, 32), (torch.int32, 8)),
                                         dev, "rules")
        for d, x in banks.items():
            banks[d] = x = sd.bank_rows(x, self.datasets[d].T, dev, "indicator bank", d)
            if host_rules is not None:
                sig.check_rules(host_rules, int(x.shape[0]), d)

        def launch(d, table):
            x = banks[d]
            _abi.check(self._lib, self._lib.gte_build_signals(
                self._h, d, C.c_void_p(x.data_ptr()), int(x.shape[0]), int(x.stride(0)),
                C.c_void_p(d_rules.data_ptr()), int(d_rules.shape[0]), C.c_void_p(table.data_ptr()),
                int(table.shape[1])))
        return sd.run_builder(self, banks, int(d_rules.shape[0]), torch.int8, sig.row_stride, launch, bind, wants_list)

    def compose_signals(self, clauses, specs, dataset=None, bind=True):
        """Compose signal tables ON THE DEVICE from clause rows (`gte_compose_signals`): one spec per
        strategy (`signals.compose`, `signals.COMPOSE_DTYPE`; the rule is stated in include/gte.h) over
        a table of clause rows int8 [R, T] of zone codes 0 / 1 / 2 — what
        ``build_signals(bank, signals.clauses(...), bind=False)`` returns, or an earlier composed table.
        Returns the table as a torch int8 [S, T] view of a padded device tensor — complete for torch to
        read when the call returns — and, with ``bind=True``, binds that same tensor as `bind_signals`
        would, without a second copy.  No [S, T] array exists on the host.

        clauses: a NumPy array or a CUDA int8 tensor [R, T] for dataset `dataset` (default: the only
        one); with ``dataset=None`` and D > 1 a list of D clause tables, one per resident dataset, and
        the result is a list of D tables.  A CUDA table whose rows are 16-byte aligned and padded to
        `signals.row_stride(T)` bytes (the ``[:, :T]`` view `build_signals` returns) is read in place.
        specs: a `COMPOSE_DTYPE` array [S], whose `n_in` and `in` are checked against R here, or a
        CUDA tensor uint8 [S, 128] of the same bytes, which is the caller's contract: the kernel gives
        a spec that names no clause row a row of -1.  One spec array serves every dataset; the
        caller's order is kept (a row index is a strategy id).  Specs that read the same clause rows
        are best placed next to each other, as the rules of `build_signals` are."""
        torch = self._torch
        if torch is None:
            raise ValueError("compose_signals needs output='torch'")
        from . import signal_device as sd, signals as sig
        dev = self._t["obs"].device
        rows, wants_list = sd.per_dataset(clauses, len(self.datasets), dataset, "clause tables")
        d_specs, host_specs = sd.records(specs, sig.COMPOSE_DTYPE, "COMPOSE_DTYPE", ((torch.uint8, 128),),
                                         dev, "specs")
        for d, x in rows.items():
            rows[d] = x = sd.table_rows(x, self.datasets[d].T, dev, "clause table", d)
            if host_specs is not None:
                sig.check_compose(host_specs, int(x.shape[0]), d)

        def launch(d, table):
            x = rows[d]
            _abi.check(self._lib, self._lib.gte_compose_signals(
                self._h, d, C.c_void_p(x.data_ptr()), int(x.shape[0]), int(x.stride(0)),
                C.c_void_p(d_specs.data_ptr()), int(d_specs.shape[0]), C.c_void_p(table.data_ptr()),
                int(table.shape[1])))
        return sd.run_builder(self, rows, int(d_specs.shape[0]), torch.int8, sig.row_stride, launch, bind, wants_list)

    def build_indicators(self, specs, dataset=None, inputs=None):
        """Build indicator banks ON THE DEVICE from the resident market data (`gte_build_indicators`):
        one row per spec (`signals.indicators`, `signals.INDICATOR_DTYPE`; what each kind computes is
        stated in include/gte.h) over the dataset's close / high / low, a static feature column, or
        a row of `inputs`.  Returns a torch f32 [C, T] view of a device tensor whose rows are padded to
        `signals.bank_stride(T)` floats — complete for torch to read when the call returns, and exactly
        the form `build_signals` reads in place: ``env.build_signals(env.build_indicators(specs),
        rules)`` copies nothing.

        specs: an `INDICATOR_DTYPE` array [C], checked here against the env (feature columns, input
        rows, whether the dataset has high / low), or a CUDA tensor uint8 [C, 16] / int32 [C, 4] of
        the same bytes, which is the caller's contract: the kernel gives a spec it cannot serve a row
        of NaN.  With ``dataset=None`` and D > 1 one spec array serves every dataset and a list of D
        banks comes back.  inputs: a NumPy array or a CUDA f32 tensor [C_in, T] (volume, or a bank an
        earlier call returned: the signal line of a MACD is an EMA of such a row), or a list of D of
        them; padded like a bank of `build_signals`, or read in place when it has that layout."""
        torch = self._torch
        if torch is None:
            raise ValueError("build_indicators needs output='torch'")
        from . import signal_device as sd, signals as sig
        dev = self._t["obs"].device
        D = len(self.datasets)
        # (the only dataset needs no list: a list is then one input bank, as nested rows)
        banks, wants_list = sd.per_dataset(inputs, D, 0 if D == 1 and dataset is None else dataset, "input banks",
                                           optional=True)
        d_specs, host_specs = sd.records(specs, sig.INDICATOR_DTYPE, "INDICATOR_DTYPE",
                                         ((torch.uint8, 16), (torch.int32, 4)), dev, "specs")
        for d, x in banks.items():
            ds = self.datasets[d]
            if x is not None:
                banks[d] = x = sd.bank_rows(x, ds.T, dev, "input bank", d)
            if host_specs is not None:
                sig.check_indicators(host_specs, ds.n_static, 0 if x is None else int(x.shape[0]),
                                     getattr(ds, "high", None) is not None, getattr(ds, "low", None) is not None, d)

        def launch(d, bank):
            x = banks[d]
            _abi.check(self._lib, self._lib.gte_build_indicators(
                self._h, d, C.c_void_p(d_specs.data_ptr()), int(d_specs.shape[0]),
                C.c_void_p(x.data_ptr()) if x is not None else None, int(x.shape[0]) if x is not None else 0,
                int(x.stride(0)) if x is not None else 0, C.c_void_p(bank.data_ptr()), int(bank.shape[1])))
        return sd.run_builder(self, banks, int(d_specs.shape[0]), torch.float32, sig.bank_stride, launch, False, wants_list)

    @property
    def num_strategies(self) -> int:
        """S of the bound signal tables (0: none bound)."""
        return int(next(iter(self._signals.values())).shape[0]) if self._signals else 0

    def _strategy(self, strategy, what):
        """`strategy` of signal_actions() / backtest_signals() as a device int32 [N] tensor or None
        (= (env_id_base + e) % S); a host array is checked against [0, S), a CUDA tensor is the
        caller's contract, as in the C ABI."""
        torch = self._torch
        if torch is None:
            raise ValueError(f"{what} needs output='torch'")
        if strategy is None:
            return None
        if not (isinstance(strategy, torch.Tensor) and strategy.is_cuda):
            a = np.asarray(strategy.cpu().numpy() if isinstance(strategy, torch.Tensor) else strategy)
            if a.dtype.kind not in "iu":
                raise TypeError("strategy must be integers")
            S = self.num_strategies
            if a.size and S and (a.min() < 0 or a.max() >= S):
                raise IndexError(f"strategy outside [0, {S})")
            strategy = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(self._t["obs"].device)
        strategy = strategy.to(torch.int32).contiguous()
        if tuple(strategy.shape) != (self.num_envs,):
            raise ValueError(f"expected strategy of shape ({self.num_envs},)")
        return strategy

    def signal_actions(self, strategy=None, out=None):
        """The action the bound signal tables give every env for its NEXT step, as an int32 [N]
        device tensor (-1 = hold): `gte_signal_actions`, one small stream-ordered launch that can be
        captured.  ``env.step(env.signal_actions())`` drives the env closed-loop by signals, with
        observations; `out` (int32 [N], CUDA, contiguous) is written instead of a new tensor."""
        strategy = self._strategy(strategy, "signal_actions")
        torch = self._torch
        dev = self._t["obs"].device
        if out is None:
            with torch.cuda.device(dev):
                out = torch.empty((self.num_envs,), dtype=torch.int32, device=dev)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32
                  and tuple(out.shape) == (self.num_envs,) and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int32 CUDA tensor of shape ({self.num_envs},)")
        self._keep_strategy = strategy  # alive until the launch has consumed it
        _abi.check(self._lib, self._lib.gte_signal_actions(
            self._h, None if strategy is None else C.c_void_p(strategy.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def backtest_signals(self, K, *, strategy=None, resume=False):
        """`backtest()` of K steps with every step's action looked up on the device in the bound
        signal tables, at the row (and dataset) the env stands on before the step
        (`gte_backtest_signals`) — so random episode starts, `max_episode_duration`, dataset
        switching and auto-reset all stay on, and no [K, N] action tensor exists.  Env e follows
        strategy ``strategy[e]`` (int32 [N]); None = ``(env_id_base + e) % S``.  Records, `resume`
        and the state afterwards are those of `backtest()`.  Returns a `BacktestStats`."""
        from .backtest_stats import BacktestStats
        if self._reward_callable is not None or self._dyn_callables:
            raise NotImplementedError("a fused backtest runs all steps on the device: custom Python "
                                      "reward / dynamic-feature callables need step()")
        strategy = self._strategy(strategy, "backtest_signals")
        ptr = C.c_void_p()
        self._keep_strategy = strategy
        _abi.check(self._lib, self._lib.gte_backtest_signals(
            self._h, None if strategy is None else C.c_void_p(strategy.data_ptr()), int(K),
            0 if resume else 1, C.byref(ptr)))
        self._stepped()
        # what this call ran with, for BacktestStats.by_strategy(): the map (None = the default one) and S
        self._backtest_map = (strategy, self.num_strategies)
        return BacktestStats(self, ptr.value)

    def backtest_curves(self, K=None, *, actions=None, strategy=None, stride=1, resume=False, valuation=True,
                        drawdown=False, reward=False, position=False, row=False, flags=True, out=None):
        """`backtest_signals(K)` — or, with ``actions=`` int32 [K, N], `backtest(actions)` — that also keeps ROWS
        (`gte_backtest_curves`): the equity curve and what goes with it, one row per `stride` steps and env, as
        [R, N] device tensors with R = ceil(K / stride), written by the same launch from the registers that hold
        the step.  Exactly one of `K` and `actions` is given; with `K` the bound signal tables decide, and the
        exit rules while they are bound.  The columns: ``valuation`` (the window's last step), ``drawdown`` (its
        deepest, against the record's running peak: the underwater curve), ``reward`` (its sum), ``position`` (the
        position index), ``row`` (the market row), ``flags`` (terminated / truncated / reset / frozen, OR-ed) —
        include/gte.h states each.  Records, `resume` and the state afterwards are those of the call without rows;
        with ``resume=False`` the maximum of an env's drawdown column is its ``stats.max_drawdown`` to the bit.
        `out`: a previous result with the same K, stride and columns, whose tensors are written again.  Not
        together with trade or period tracking.  Returns a `Curves` (its ``stats`` is the `BacktestStats`)."""
        from . import curves as cv
        from .backtest_stats import BacktestStats
        torch = self._torch
        if (K is None) == (actions is None):
            raise TypeError("backtest_curves takes either K (steps by the bound signal tables) or actions=")
        if isinstance(stride, bool) or int(stride) != stride:
            raise TypeError("stride must be an integer")
        if actions is not None:
            if strategy is not None:
                raise TypeError("strategy goes with K (signal tables), not with actions=")
            actions = self._sequence_actions(actions, "backtest_curves")
            K = int(actions.shape[0])
        else:
            if self._reward_callable is not None or self._dyn_callables:
                raise NotImplementedError("a fused backtest runs all steps on the device: custom Python "
                                          "reward / dynamic-feature callables need step()")
            strategy = self._strategy(strategy, "backtest_curves")
            K = int(K)
        if K < 1:
            raise ValueError("backtest_curves: K must be >= 1")
        keep = dict(valuation=valuation, drawdown=drawdown, reward=reward, position=position, row=row, flags=flags)
        dev = self._t["obs"].device
        cols = {}
        if int(stride) >= 1:  # (else the library refuses below, with its message)
            cols = cv.take_out(torch, out, cv.column_shapes(torch, keep, K, int(stride), self.num_envs), dev)
        b = _abi.GteCurveBufs()
        for c, t in cols.items():
            setattr(b, c, t.data_ptr())
        ptr = C.c_void_p()
        self._keep = (actions, cols)  # alive until the launch has consumed them
        self._keep_strategy = strategy
        _abi.check(self._lib, self._lib.gte_backtest_curves(
            self._h, None if actions is None else C.c_void_p(actions.data_ptr()),
            None if strategy is None else C.c_void_p(strategy.data_ptr()), K, int(stride), 0 if resume else 1,
            C.byref(b), C.byref(ptr)))
        self._stepped()
        # (as after backtest() / backtest_signals(): what by_strategy() maps with)
        self._backtest_map = None if actions is not None else (strategy, self.num_strategies)
        return cv.Curves(self, cols, BacktestStats(self, ptr.value), K, int(stride))

    # -- exit rules: stop-loss, trailing stop, take-profit and time exits per strategy --------
    def bind_exits(self, rules, rule_of_env=None):
        """Bind exit rules (`gte_bind_exit_rules`): while they are bound, `signal_actions()` and
        `backtest_signals()` let every env leave for its rule's `exit_position` when its OWN path
        trips a stop-loss, a trailing stop, a take-profit or a time limit, and hold until the signal
        moves; otherwise the table decides as before (the rule is stated in include/gte.h).  The fused
        backtest keeps each env's exit state in registers through all its steps.

        rules: an `EXIT_DTYPE` array [R] (`signals.exit_rules`), whose `exit_position` is checked
        against `positions` here, or a CUDA tensor uint8 [R, 32] / int32 [R, 8] of the same bytes,
        which is the caller's contract: a rule whose exit_position names no position is off.
        rule_of_env: int32 [N] with values in [0, R) — a host array is checked, a CUDA tensor is the
        caller's contract — or None: env e follows rule ``strategy_of(e) % R``.  Every call starts
        the exit state afresh (the next decision sees a reset row).  ``rules=None`` unbinds."""
        torch = self._torch
        if torch is None:
            raise ValueError("bind_exits needs output='torch'")
        ptr = C.c_void_p()
        if rules is None:
            if rule_of_env is not None:
                raise ValueError("rule_of_env without rules")
            _abi.check(self._lib, self._lib.gte_bind_exit_rules(self._h, None, 0, None, C.byref(ptr)))
            self._exits = None
            return
        from . import signal_device as sd, signals as sig
        dev = self._t["obs"].device
        d_rules, host = sd.records(rules, sig.EXIT_DTYPE, "EXIT_DTYPE", ((torch.uint8, 32), (torch.int32, 8)),
                                   dev, "rules")
        if host is not None:
            sig.check_exit_rules(host, len(self.positions))
        R = int(d_rules.shape[0])
        d_map = None
        if rule_of_env is not None:
            if isinstance(rule_of_env, torch.Tensor) and rule_of_env.is_cuda:
                d_map = rule_of_env.to(device=dev, dtype=torch.int32).contiguous()
            else:
                a = np.asarray(rule_of_env.numpy() if isinstance(rule_of_env, torch.Tensor) else rule_of_env)
                if a.dtype.kind not in "iu":
                    raise TypeError("rule_of_env must be integers")
                if a.size and (a.min() < 0 or a.max() >= R):
                    raise IndexError(f"rule_of_env outside [0, {R})")
                d_map = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
            if tuple(d_map.shape) != (self.num_envs,):
                raise ValueError(f"expected rule_of_env of shape ({self.num_envs},)")
        torch.cuda.current_stream(dev).synchronize()  # the copies above: the env may launch on another stream
        _abi.check(self._lib, self._lib.gte_bind_exit_rules(
            self._h, C.c_void_p(d_rules.data_ptr()), R, None if d_map is None else C.c_void_p(d_map.data_ptr()),
            C.byref(ptr)))
        self._exits = (d_rules, d_map)
        self._exit_state_ptr = int(ptr.value or 0)

    @property
    def num_exit_rules(self) -> int:
        """R of the bound exit rules (0: none bound)."""
        return int(self._exits[0].shape[0]) if self._exits else 0

    def exit_state(self):
        """The per-env exit state (`gte_exit_state`, include/gte.h) as an `ExitState` of device views;
        needs a `bind_exits` before it."""
        from .exit_state import ExitState
        if not self._exit_state_ptr:
            raise ValueError("exit_state() before bind_exits(): the env has no exit state yet")
        return ExitState(self, self._exit_state_ptr)

    # -- misc ---------------------------------------------------------------------------
    def synchronize(self):
        _abi.check(self._lib, self._lib.gte_synchronize(self._h))

    def launch_info(self) -> dict:
        v = [C.c_int32() for _ in range(4)]
        _abi.check(self._lib, self._lib.gte_get_launch_info(self._h, *[C.byref(x) for x in v]))
        d = dict(zip(("envs_per_wave", "threads_per_block", "n_blocks", "vector_bytes"),
                     (x.value for x in v)))
        flags, d["vector_bytes"] = divmod(d["vector_bytes"], 1000)
        d["phase_a"] = "cooperative" if flags & 1 else "per-wave"
        d["dyn_columns"] = ("global", "lds-raw-rings", "lds-resolved")[(flags >> 1) & 3]
        d["structure"] = "phase A, LDS barrier, gather"
        d["obs_stores"] = ("plain", "non-temporal", "sc1", "?")[(flags >> 4) & 3]
        d["resident_workgroups_per_cu"] = (flags >> 6) & 15
        # the launches that store one row per env (gte.h, GTE_SLIDE_STORE); obs_stores while the env does not slide
        d["slide_obs_stores"] = ("plain", "non-temporal", "sc1", "?")[(flags >> 10) & 3]
        return d

    def timer_start(self):
        _abi.check(self._lib, self._lib.gte_timer_start(self._h))

    def timer_mark(self):
        """Record the end of the timed span now, without waiting (read it with `timer_stop`)."""
        _abi.check(self._lib, self._lib.gte_timer_stop(self._h, None))

    def timer_stop(self) -> float:
        ms = C.c_float()
        _abi.check(self._lib, self._lib.gte_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def close(self, **kwargs):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.gte_destroy(self._h)
            self._h = C.c_void_p()
        self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
