"""tests/layouts.py on CPU tensors: every layout holds the values asked for, poisons the
rest of its storage, and lands in the kernel family its name claims -- the check that the
GPU layout tests (test_gpu_layouts*.py) feed the kernels what they mean to feed them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from layouts import LAYOUTS, layout_view

# host dtype -> (elements per 16-byte vector, torch dtype of the view, V)
KINDS = {"u32": (np.uint32, 4, torch.int32, 24), "u64": (np.uint64, 2, torch.int64, 12),
         "f32": (np.float32, 4, torch.float32, 24), "bf16": (np.uint16, 8, torch.bfloat16, 24)}
SCALAR = {"pad_odd", "offset_1"}                 # the layouts the scalar kernels take although V % vw == 0
T, B = 5, 3


def _values(kind):
    dt, vw, _, V = KINDS[kind]
    assert V % vw == 0
    rng = np.random.default_rng(V + vw)
    if kind == "f32":
        return rng.standard_normal((T, B, V)).astype(np.float32)
    if kind == "bf16":
        return (rng.standard_normal((T, B, V)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return rng.integers(1, 1 << 20, size=(T, B, V)).astype(dt)


def _bits(t):
    """A tensor's bit patterns as an unsigned numpy array."""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(it).numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t.element_size()])


def _is_vector(ptr, V, step_stride, stream_stride, vw):
    """The rule of include/lac.h and encode_dispatch (lac_encode.hip) / decode_plan
    (lac_select.h): 16-byte loads iff the base is 16-byte aligned and V and both strides
    are multiples of the vector width; the logits entry points refuse everything else."""
    return ptr % 16 == 0 and V % vw == 0 and step_stride % vw == 0 and stream_stride % vw == 0


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_layout_values_poison_and_class(kind, name):
    dt, vw, tdt, V = KINDS[kind]
    x = _values(kind)
    v = layout_view(x, "cpu", name)
    assert v.dtype == tdt and tuple(v.shape) == (T, B, V) and v.stride(2) == 1
    want = x
    if name == "step_bcast":
        want = np.broadcast_to(x[:1], x.shape)
    elif name == "stream_bcast":
        want = np.broadcast_to(x[:, :1], x.shape)
    assert np.array_equal(_bits(v), want.view(_bits(v).dtype))
    # the storage: as many elements as the layout's table says, the view's ones are the
    # values, every other one is poison
    es = v.element_size()
    store = torch.empty(0, dtype=tdt).set_(v.untyped_storage())
    size = {"contig": T * B * V, "pad_vec": T * B * (V + 3 * vw), "pad_odd": T * B * (V + 1),
            "step_pad": T * (B + 1) * V, "transposed": T * B * V, "offset_vec": T * B * V + 2 * vw,
            "offset_1": T * B * V + vw, "step_bcast": B * (V + vw), "stream_bcast": T * V}[name]
    assert store.numel() == size
    inside = np.zeros(size, dtype=bool)
    off0 = (v.data_ptr() - store.data_ptr()) // es
    idx = (off0 + np.arange(T)[:, None, None] * v.stride(0) + np.arange(B)[None, :, None] * v.stride(1)
           + np.arange(V)[None, None, :])
    inside[idx.ravel()] = True
    distinct = {"step_bcast": B * V, "stream_bcast": T * V}.get(name, T * B * V)
    assert int(inside.sum()) == distinct
    sb = _bits(store)
    poison = {"u32": 0xFFFFFFFF, "u64": 0xFFFFFFFFFFFFFFFF, "f32": 0x7F800000, "bf16": 0x7F80}[kind]
    assert (sb[~inside] == poison).all()
    if kind in ("f32", "bf16"):
        assert torch.isposinf(store.float()[torch.from_numpy(~inside)]).all()
    assert not (_bits(v) == poison).any()                           # no value is mistaken for poison
    # strides as BatchCoder passes them, and the family they select
    step_stride = v.stride(0) if T > 1 else 0
    stream_stride = v.stride(1) if B > 1 else 0
    strides = {"contig": (B * V, V), "pad_vec": (B * (V + 3 * vw), V + 3 * vw), "pad_odd": (B * (V + 1), V + 1),
               "step_pad": ((B + 1) * V, V), "transposed": (V, T * V), "offset_vec": (B * V, V),
               "offset_1": (B * V, V), "step_bcast": (0, V + vw), "stream_bcast": (V, 0)}[name]
    assert (step_stride, stream_stride) == strides
    assert store.data_ptr() % 16 == 0
    assert off0 == {"offset_vec": vw, "offset_1": 1}.get(name, 0)
    vec = _is_vector(v.data_ptr(), V, step_stride, stream_stride, vw)
    assert vec == (name not in SCALAR), (v.data_ptr() % 16, step_stride % vw, stream_stride % vw)
    if name == "pad_odd":
        assert v.data_ptr() % 16 == 0 and stream_stride % vw != 0   # scalar by its strides alone
    if name == "offset_1":
        assert v.data_ptr() % 16 == es and stream_stride % vw == 0  # scalar by its base alone
    # the slices the GPU tests cut keep the class: a leading-axis slice moves the base by
    # whole rows
    for a in (1, 2):
        s = v[a:]
        assert _is_vector(s.data_ptr(), V, s.stride(0) if s.shape[0] > 1 else 0, stream_stride, vw) == vec


def test_unknown_layout_is_refused():
    with pytest.raises(ValueError):
        layout_view(np.ones((1, 1, 4), dtype=np.uint32), "cpu", "nope")
