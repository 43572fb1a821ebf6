"""Non-default memory layouts for the tables and logits the library takes as a base
pointer and two element strides (include/lac.h: row (t, b) at t*step_stride +
b*stream_stride; a stride of 0 re-uses the row).

``layout_view(values, device, name)`` puts the host array ``values`` [T, B, V] into a
larger storage and returns a torch view of shape [T, B, V] over it.  Every storage element
outside the view is poison -- all-ones table entries (one extra entry read pushes a row
total up, or over 2^64), +inf logits (one read changes the row maximum and with it the
whole table) -- so a kernel that reads a wrong row, reads past V or steps by the wrong
stride computes different bits or fails; it cannot be right by luck.

``vw`` is the width of a 16-byte vector in elements (4 u32 / f32, 2 u64, 8 bf16):

    contig        [T,B,V]                              baseline
    pad_vec       [T,B,V+3*vw][..., :V]                vector kernels, stream_stride != V
    pad_odd       [T,B,V+1][..., :V]                   V % vw == 0 but odd strides: scalar kernels
    step_pad      [T,B+1,V][:, :B]                     step_stride != B*stream_stride
    transposed    [B,T,V].transpose(0, 1)              step_stride < stream_stride
    offset_vec    flat buffer, view starts vw elements in   aligned base, not an allocation start
    offset_1      flat buffer, view starts 1 element in     misaligned base: scalar kernels
    step_bcast    [1,B,V+vw][..., :V].expand(T, ...)   static rows per stream, padded stream stride
    stream_bcast  [T,1,V].expand(-1, B, -1)            stream_stride == 0, step_stride != 0

The two broadcasts hold values[:1] / values[:, :1]; what a layout is expected to give is
always the oracle's result on the view's materialised values (``view.contiguous().cpu()``).
"""
import numpy as np

LAYOUTS = ("contig", "pad_vec", "pad_odd", "step_pad", "transposed", "offset_vec", "offset_1", "step_bcast",
           "stream_bcast")
# host dtype -> (elements per 16-byte vector, poison, numpy dtype torch can take, torch dtype name)
_KINDS = {
    np.dtype(np.uint32): (4, 0xFFFFFFFF, np.int32, "int32"),
    np.dtype(np.uint64): (2, 0xFFFFFFFFFFFFFFFF, np.int64, "int64"),
    np.dtype(np.float32): (4, np.inf, np.float32, "float32"),
    np.dtype(np.uint16): (8, 0x7F80, np.int16, "bfloat16"),         # bf16 bit patterns; 0x7F80 = +inf
}


def layout_view(values, device, name):
    """values: host array [T, B, V] of uint32 / uint64 tables, float32 logits or uint16
    (bf16 bit patterns) logits -> torch view [T, B, V] (int32 / int64 / float32 / bfloat16)
    on ``device`` in layout ``name``, everything around it poisoned."""
    import torch
    values = np.asarray(values)
    vw, poison, carrier, tname = _KINDS[values.dtype]
    T, B, V = values.shape
    n = T * B * V
    # storage shape, and the view as one expression over numpy and torch alike
    if name == "contig":
        shape, cut = (T, B, V), lambda s: s
    elif name == "pad_vec":
        shape, cut = (T, B, V + 3 * vw), lambda s: s[..., :V]
    elif name == "pad_odd":
        shape, cut = (T, B, V + 1), lambda s: s[..., :V]
    elif name == "step_pad":
        shape, cut = (T, B + 1, V), lambda s: s[:, :B]
    elif name == "transposed":
        shape, cut = (B, T, V), lambda s: s.swapaxes(0, 1)
    elif name == "offset_vec":
        shape, cut = (n + 2 * vw,), lambda s: s[vw:vw + n].reshape(T, B, V)
    elif name == "offset_1":
        shape, cut = (n + vw,), lambda s: s[1:1 + n].reshape(T, B, V)
    elif name == "step_bcast":
        shape, cut = (1, B, V + vw), lambda s: s[..., :V]
        values = values[:1]
    elif name == "stream_bcast":
        shape, cut = (T, 1, V), lambda s: s
        values = values[:, :1]
    else:
        raise ValueError(f"unknown layout {name!r}")
    host = np.full(shape, poison, dtype=values.dtype)
    cut(host)[...] = values
    dev = torch.from_numpy(host.view(carrier)).to(device)
    if tname == "bfloat16":
        dev = dev.view(torch.bfloat16)
    return cut(dev).expand(T, B, V)
