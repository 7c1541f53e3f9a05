"""The torch side of the signal pipeline (`BatchedTradingEnv.build_signals`, `compose_signals`,
`build_indicators`): how their arguments reach the device and how their results come back.  One
decision lives here — the device layout of a per-dataset table of rows: rows padded to
`signals.row_stride(T)` / `signals.bank_stride(T)` elements, a 16-byte aligned base, and when a
caller's tensor already has that layout and is read in place (`_rows`) — together with the "one
item, or one per dataset" convention of the arguments (`per_dataset`).  The host half of the layout
is `signals.py`; the C half is checked in gte_api.hip (`check_stride`).  Plain functions: the env
keeps its state."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import signals as sig


def per_dataset(arg, D: int, dataset, what: str, optional: bool = False):
    """`arg` of a call over D resident datasets -> ({d: item}, wants_list).  ``dataset=d``: `arg` is
    the item of dataset d.  ``dataset=None``: a list or tuple of D items, one per dataset, and the
    caller gets a list back; with D == 1 also the item itself.  `optional`: None is no item for any
    dataset (a list comes back when there are several)."""
    if dataset is not None:
        if not 0 <= int(dataset) < D:
            raise IndexError(f"dataset {dataset} out of range")
        return {int(dataset): arg}, False
    if arg is None and optional:
        return {d: None for d in range(D)}, D > 1
    many = isinstance(arg, (list, tuple))
    if many and len(arg) == D:
        return dict(enumerate(arg)), True
    if D == 1 and not many:
        return {0: arg}, False
    raise ValueError(f"expected a list of {D} {what}, one per dataset (or dataset=d)")


def records(x, dtype: np.dtype, dtype_name: str, forms, device, name: str):
    """Spec records on the device -> (tensor [n, width], host array or None).  `x` is a
    one-dimensional array of the structured `dtype` (signals.<dtype_name>), which also comes back as
    the host copy the caller checks, or a contiguous tensor on the env's kind of device in one of
    `forms` — (torch dtype, width) pairs that spell the same bytes — which is taken as it is."""
    if isinstance(x, torch.Tensor):
        if not (x.device.type == device.type and x.dim() == 2 and x.is_contiguous()
                and (x.dtype, int(x.shape[1])) in forms):
            shapes = " / ".join(f"{str(t).split('.')[-1]} [n, {w}]" for t, w in forms)
            raise TypeError(f"{name}: an array of signals.{dtype_name}, or a contiguous device tensor {shapes}")
        d_x, host = x.to(device), None
    else:
        host = np.ascontiguousarray(x)
        if host.dtype != dtype or host.ndim != 1:
            raise TypeError(f"{name}: a one-dimensional array of signals.{dtype_name}")
        d_x = torch.from_numpy(host.view(np.uint8).reshape(-1, dtype.itemsize).copy()).to(device)
    if int(d_x.shape[0]) < 1:
        raise ValueError(f"{name}: the call needs at least one record")
    return d_x, host


def _rows(x, T: int, dtype, fill, stride_of, pad_host, device, what: str, d: int):
    """Operand rows on the device -> a [rows, T] view of a `dtype` tensor in the padded layout: unit
    column stride, a row stride of whole 16-byte pieces that is at least ``stride_of(T)``, a 16-byte
    aligned base.  A tensor on the env's kind of device that has the layout is that view; any other
    one is copied into a fresh tensor of row stride ``stride_of(T)`` whose padding holds `fill`.
    Anything else is a host operand and goes through `pad_host`."""
    if isinstance(x, torch.Tensor) and x.device.type == device.type:
        if x.dim() != 2 or x.dtype != dtype:
            raise TypeError(f"{what}: a two-dimensional {str(dtype).split('.')[-1]} tensor is expected")
        x = x.to(device)
    else:
        host = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
        x = torch.from_numpy(pad_host(host)).to(device)[:, :host.shape[-1]]
    if int(x.shape[1]) != T:
        raise ValueError(f"{what} of dataset {d} has {int(x.shape[1])} columns, the dataset {T} rows")
    if int(x.shape[0]) < 1:
        raise ValueError(f"{what} needs at least one row")
    piece = sig.PIECE // x.element_size()
    if x.stride(1) == 1 and x.stride(0) % piece == 0 and x.stride(0) >= stride_of(T) and x.data_ptr() % sig.PIECE == 0:
        return x
    with torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext():
        buf = torch.full((int(x.shape[0]), stride_of(T)), fill, dtype=dtype, device=device)
    buf[:, :T] = x
    return buf[:, :T]


def table_rows(x, T: int, device, what: str, d: int):
    """int8 rows (a clause table): padding -1, `signals.row_stride`; a host operand goes through
    `signals.as_int8_table` and `signals.pad_rows`."""
    return _rows(x, T, torch.int8, -1, sig.row_stride, lambda a: sig.pad_rows(sig.as_int8_table(a)),
                 device, what, d)


def bank_rows(x, T: int, device, what: str, d: int):
    """float32 rows (an indicator or input bank): padding 0, `signals.bank_stride`; a host operand
    goes through `signals.pad_bank`, so a one-dimensional array is one row."""
    return _rows(x, T, torch.float32, 0, sig.bank_stride, sig.pad_bank, device, what, d)


def run_builder(env, which, rows: int, dtype, stride_of, launch, bind: bool, wants_list: bool):
    """The launch-and-return tail of a builder: allocate one padded [rows, stride_of(T)] output per
    dataset of `which` on the env's device, run ``launch(d, out)`` (the ABI call) for each, and
    return the [rows, T] views — a list in the order of `which`, or the only one.  `bind`: the
    outputs are signal tables and get bound, refused before anything runs if they would not agree
    with the tables that stay bound."""
    dev = env._t["obs"].device
    with torch.cuda.device(dev):
        out = {d: torch.empty((rows, stride_of(env.datasets[d].T)), dtype=dtype, device=dev) for d in which}
    if bind:
        env._check_one_s(out, out)
    torch.cuda.current_stream(dev).synchronize()  # the copies of the operands: the env may launch on another stream
    for d, buf in out.items():
        launch(d, buf)
    env.synchronize()  # the outputs are complete: for torch on any stream, and before the inputs go
    if bind:
        for d, buf in out.items():
            env._bind_padded(d, buf)
    views = [buf[:, :env.datasets[d].T] for d, buf in out.items()]
    return views if wants_list else views[0]
