"""The torch side of the signal pipeline over CPU tensors: when an operand is read in place and when
it is copied into the padded layout, the per-dataset argument convention, the record forms, and the
spec checks of signals.py — the decisions of signal_device.py that the GPU tests only see the
results of."""
import numpy as np
import pytest
import torch

from gym_trading_env_amd import signal_device as sd
from gym_trading_env_amd import signals

CPU = torch.device("cpu")
ROWS = 3
#: (rows function, torch dtype, fill, host padder, element size)
KINDS = {"table": (sd.table_rows, torch.int8, -1, signals.pad_rows, 1),
         "bank": (sd.bank_rows, torch.float32, 0, signals.pad_bank, 4)}


def _values(shape, dtype):
    n = int(np.prod(shape))
    return (torch.arange(n) % 5).reshape(shape).to(dtype)


def _aligned(rows, stride, dtype, offset=0):
    """a [rows, stride] tensor whose base is `offset` elements past a 16-byte boundary, filled with 9"""
    esz = torch.empty(0, dtype=dtype).element_size()
    flat = torch.full((rows * stride + 32,), 9, dtype=dtype)
    skip = (-flat.data_ptr() % 16) // esz + offset
    t = flat[skip:skip + rows * stride].view(rows, stride)
    assert t.data_ptr() % 16 == offset * esz % 16
    return t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,width", [(37, 48), (37, 64), (48, 48), (48, 64)])
def test_a_tensor_in_the_padded_layout_is_read_in_place(kind, T, width):
    rows_of, dtype, _, _, _ = KINDS[kind]
    x = _aligned(ROWS, width, dtype)[:, :T]
    x.copy_(_values((ROWS, T), dtype))
    got = rows_of(x, T, CPU, "operand", 0)
    assert got.data_ptr() == x.data_ptr() and got.stride() == x.stride() == (width, 1)
    assert tuple(got.shape) == (ROWS, T) and torch.equal(got, x)


def _copied_inputs(T, dtype):
    """tensors [ROWS, T] that lack the layout, by what they lack"""
    stride = signals.row_stride(T)
    # 56 int8 / 50 float32: above the minimum of 48, but no whole number of 16-byte pieces
    ragged = 56 if dtype == torch.int8 else 50
    cases = {"base off by one element": _aligned(ROWS, stride, dtype, offset=1)[:, :T],
             "column stride 2": _aligned(ROWS, 2 * stride, dtype)[:, :2 * T:2],
             "row stride not whole pieces": _aligned(ROWS, ragged, dtype)[:, :T]}
    if T == 37:
        cases["contiguous, rows not padded"] = _aligned(ROWS, T, dtype)
        cases["row stride 40: below the minimum (and for int8 not whole pieces)"] = _aligned(ROWS, 40, dtype)[:, :T]
    return cases


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [37, 48])
def test_a_tensor_without_the_layout_is_copied_into_it(kind, T):
    rows_of, dtype, fill, _, esz = KINDS[kind]
    stride = signals.row_stride(T)
    assert stride == 48
    for what, x in _copied_inputs(T, dtype).items():
        x.copy_(_values((ROWS, T), dtype))
        lo, hi = x.data_ptr(), x.data_ptr() + esz * ((ROWS - 1) * x.stride(0) + (T - 1) * x.stride(1) + 1)
        got = rows_of(x, T, CPU, "operand", 0)
        assert not lo <= got.data_ptr() < hi, what                       # new storage
        assert got.stride() == (stride, 1) and got.data_ptr() % 16 == 0, what
        assert tuple(got.shape) == (ROWS, T) and got.dtype == dtype and torch.equal(got, x), what
        whole = torch.as_strided(got, (ROWS, stride), (stride, 1))
        assert (whole[:, T:] == fill).all(), what


@pytest.mark.parametrize("T", [37, 48])
def test_host_operands_take_the_bytes_of_the_numpy_padders(T):
    stride = signals.row_stride(T)
    table = (np.arange(ROWS * T).reshape(ROWS, T) % 7 - 1).astype(np.int64)
    for x in (table, table.astype(np.int8), table.tolist(), table.astype(np.int16)):
        got = sd.table_rows(x, T, CPU, "clause table", 0)
        whole = torch.as_strided(got, (ROWS, stride), (stride, 1))
        assert got.dtype == torch.int8 and tuple(got.shape) == (ROWS, T) and got.data_ptr() % 16 == 0
        np.testing.assert_array_equal(whole.numpy(), signals.pad_rows(table.astype(np.int8)))
    bank = np.arange(ROWS * T, dtype=np.float64).reshape(ROWS, T) / 8
    for x, rows in ((bank, ROWS), (bank.astype(np.float32), ROWS), (bank.tolist(), ROWS), (table, ROWS),
                    (bank[1], 1)):
        got = sd.bank_rows(x, T, CPU, "indicator bank", 0)
        whole = torch.as_strided(got, (rows, stride), (stride, 1))
        assert got.dtype == torch.float32 and tuple(got.shape) == (rows, T) and got.data_ptr() % 16 == 0
        assert whole.numpy().tobytes() == signals.pad_bank(x).tobytes()


def test_operand_refusals():
    ok_t, ok_b = torch.zeros((ROWS, 37), dtype=torch.int8), torch.zeros((ROWS, 37), dtype=torch.float32)
    with pytest.raises(TypeError, match="int8"):
        sd.table_rows(ok_b, 37, CPU, "clause table", 0)
    with pytest.raises(TypeError, match="float32"):
        sd.bank_rows(ok_b.double(), 37, CPU, "indicator bank", 0)
    with pytest.raises(TypeError, match="float32"):
        sd.bank_rows(ok_t, 37, CPU, "indicator bank", 0)
    with pytest.raises(TypeError, match="two-dimensional"):
        sd.table_rows(ok_t[0], 37, CPU, "clause table", 0)
    with pytest.raises(TypeError, match="two-dimensional"):
        sd.bank_rows(ok_b[None], 37, CPU, "indicator bank", 0)
    with pytest.raises(TypeError):
        sd.table_rows(np.zeros((ROWS, 37)), 37, CPU, "clause table", 0)   # (as_int8_table: not integers)
    for rows_of, ok in ((sd.table_rows, ok_t), (sd.bank_rows, ok_b)):
        for x in (ok, ok.numpy()):
            with pytest.raises(ValueError, match="columns"):
                rows_of(x, 38, CPU, "operand", 1)
            with pytest.raises(ValueError, match="columns"):
                rows_of(x, 36, CPU, "operand", 1)
        with pytest.raises(ValueError, match="at least one row"):
            rows_of(ok[:0], 37, CPU, "operand", 0)


def test_per_dataset_arguments():
    a, b = object(), object()
    # one dataset: the item, or a list of one — and only the list asks for a list back
    assert sd.per_dataset(a, 1, None, "things") == ({0: a}, False)
    assert sd.per_dataset([a], 1, None, "things") == ({0: a}, True)
    assert sd.per_dataset((a,), 1, None, "things") == ({0: a}, True)
    assert sd.per_dataset(a, 1, 0, "things") == ({0: a}, False)
    assert sd.per_dataset([a], 1, 0, "things") == ({0: [a]}, False)      # dataset=d: the list is the item
    with pytest.raises(ValueError, match="list of 1 things"):
        sd.per_dataset([a, b], 1, None, "things")
    # two datasets: a list of two, or dataset=d
    assert sd.per_dataset([a, b], 2, None, "things") == ({0: a, 1: b}, True)
    assert sd.per_dataset(a, 2, 1, "things") == ({1: a}, False)
    assert sd.per_dataset([a, b], 2, 1, "things") == ({1: [a, b]}, False)
    for wrong in (a, [a], [a, b, a]):
        with pytest.raises(ValueError, match="list of 2 things"):
            sd.per_dataset(wrong, 2, None, "things")
    for D, dataset in ((1, 1), (1, -1), (2, 2), (2, -1)):
        with pytest.raises(IndexError, match="out of range"):
            sd.per_dataset(a, D, dataset, "things")
    # the operand that may be absent: no item for any dataset, a list back when there are several
    assert sd.per_dataset(None, 1, None, "things", optional=True) == ({0: None}, False)
    assert sd.per_dataset(None, 2, None, "things", optional=True) == ({0: None, 1: None}, True)
    assert sd.per_dataset(None, 2, 1, "things", optional=True) == ({1: None}, False)
    with pytest.raises(ValueError, match="list of 2"):
        sd.per_dataset(None, 2, None, "things")
    # build_indicators' rule — a list is per dataset only with several of them — is dataset=0 for the only one
    assert sd.per_dataset([a, b], 1, 0, "things", optional=True) == ({0: [a, b]}, False)


RECORDS = {
    "rules": (signals.RULE_DTYPE, "RULE_DTYPE", ((torch.uint8, 32), (torch.int32, 8)), signals.rules([0, 1, 2], b=1),
              (torch.int16, 16)),
    "compose": (signals.COMPOSE_DTYPE, "COMPOSE_DTYPE", ((torch.uint8, 128),),
                signals.compose([[0, 1], [1, 2]], np.zeros((3, 3), np.int8)), (torch.int32, 32)),
    "indicators": (signals.INDICATOR_DTYPE, "INDICATOR_DTYPE", ((torch.uint8, 16), (torch.int32, 4)),
                   signals.indicators(["sma", "ema"], n=5), (torch.int16, 8)),
}


@pytest.mark.parametrize("which", RECORDS)
def test_records(which):
    dtype, dtype_name, forms, rec, refused = RECORDS[which]
    raw = rec.view(np.uint8).reshape(len(rec), dtype.itemsize)
    rec.flags.writeable = False                                          # (a read-only array is taken too)
    t, host = sd.records(rec, dtype, dtype_name, forms, CPU, "specs")
    assert t.dtype == torch.uint8 and tuple(t.shape) == raw.shape and t.is_contiguous()
    np.testing.assert_array_equal(t.numpy(), raw)
    assert host.dtype == dtype and host.tobytes() == rec.tobytes()
    assert not np.shares_memory(t.numpy(), rec)
    t, host = sd.records(rec[::2], dtype, dtype_name, forms, CPU, "specs")   # a strided array: made contiguous
    np.testing.assert_array_equal(t.numpy(), raw[::2])
    for bad in (raw, rec.view(np.uint8), rec.reshape(1, -1), np.zeros((3, 8), np.int32)):
        with pytest.raises(TypeError, match=dtype_name):
            sd.records(bad, dtype, dtype_name, forms, CPU, "specs")
    with pytest.raises(ValueError, match="needs at least one"):
        sd.records(rec[:0], dtype, dtype_name, forms, CPU, "specs")
    for tdtype, width in forms:
        x = torch.from_numpy(raw.copy()).view(tdtype)
        assert tuple(x.shape) == (len(rec), width)
        t, host = sd.records(x, dtype, dtype_name, forms, CPU, "specs")
        assert host is None and t.data_ptr() == x.data_ptr()
        with pytest.raises(TypeError, match=dtype_name):
            sd.records(x.t(), dtype, dtype_name, forms, CPU, "specs")           # not contiguous, wrong width
        with pytest.raises(TypeError, match=dtype_name):
            sd.records(x.reshape(-1), dtype, dtype_name, forms, CPU, "specs")   # one-dimensional
        with pytest.raises(ValueError, match="needs at least one"):
            sd.records(x[:0], dtype, dtype_name, forms, CPU, "specs")
    x = torch.from_numpy(raw.copy()).view(refused[0])
    assert tuple(x.shape) == (len(rec), refused[1])
    with pytest.raises(TypeError, match=dtype_name):
        sd.records(x, dtype, dtype_name, forms, CPU, "specs")


def test_check_rules():
    signals.check_rules(signals.rules([0, 5], b=[-1, 5]), 6, 0)
    for a, b in ((6, -1), (-1, 0), (0, 6), (0, -2)):
        with pytest.raises(IndexError, match="outside the 6 rows of dataset 1"):
            signals.check_rules(signals.rules([0, a], b=[0, b]), 6, 1)


def test_check_compose():
    lut = np.zeros((3, 3), np.int8)
    ok = signals.compose([[0, 4], [4, 0]], lut)
    signals.check_compose(ok, 5, 0)
    beyond = ok.copy()
    beyond["in"][1, 2] = 99                                              # past n_in: not read, not checked
    signals.check_compose(beyond, 5, 0)
    for n_in in (0, 5):
        bad = ok.copy()
        bad["n_in"][1] = n_in
        with pytest.raises(ValueError, match="n_in"):
            signals.check_compose(bad, 5, 0)
    for row in (5, -1):
        with pytest.raises(IndexError, match="outside the 5 rows of dataset 1"):
            signals.check_compose(signals.compose([[0, 1], [row, 0]], lut), 5, 1)


def test_check_indicators():
    ok = signals.indicators(["value", "sma", "max", "min", "ema"], n=[0, 5, 4096, 3, 2],
                            source=["close", "feature", "high", "low", "input"], column=[0, 6, 0, 0, 1])
    signals.check_indicators(ok, 7, 2, True, True, 0)

    def refused(match, n_static=7, n_inputs=2, high=True, low=True, **fields):
        bad = ok.copy()
        for k, (i, v) in fields.items():
            bad[k][i] = v
        with pytest.raises(ValueError, match=match):
            signals.check_indicators(bad, n_static, n_inputs, high, low, 1)
    refused("unknown kind or source", kind=(1, len(signals.IND_KINDS)))
    refused("unknown kind or source", source=(1, -1))
    refused("window outside", n=(1, 0))
    refused("window outside", n=(2, 4097))
    refused("feature columns outside the 6 static", n_static=6)
    refused("input rows outside the 1 rows of dataset 1", n_inputs=1)
    refused("input rows outside the 0 rows", n_inputs=0)
    refused("read high, which dataset 1 does not have", high=False)
    refused("read low, which dataset 1 does not have", low=False)
    signals.check_indicators(ok[:2], 7, 0, False, False, 0)              # what is not read may be absent
