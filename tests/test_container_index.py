"""container._index -- the header and count table decompress_batch reads without slicing the
streams -- agrees with container.unpack and raises what it raises.  No GPU needed."""
import struct

import numpy as np
import pytest

from lac_amd import container


def _blob(n_bits, **kw):
    rng = np.random.default_rng(len(n_bits))
    streams = [rng.integers(0, 256, (L + 7) // 8, dtype=np.uint8).tobytes() for L in n_bits]
    return container.pack(streams, list(range(len(n_bits))), n_bits, 48, 999, **kw), streams


@pytest.mark.parametrize("n_bits", [[0], [1, 0, 7, 8, 9, 63, 64, 65], [0, 0, 0], list(range(0, 700, 13))])
def test_index_agrees_with_unpack(n_bits):
    blob, streams = _blob(n_bits, mapping="floor", pmf_bits=64, q1_logits=True)
    want = container.unpack(blob)
    h, n_symbols, nb, body = container._index(blob)
    assert {k: want[k] for k in h} == h
    assert n_symbols.tolist() == want["n_symbols"] and nb.tolist() == want["n_bits"]
    assert bytes(body) == b"".join(streams)


def test_index_raises_what_unpack_raises():
    blob, _ = _blob([9, 64, 3])
    for bad in (blob + b"\0", blob[:-1], b"LAC2" + blob[4:], blob[:4] + b"\x02\x00" + blob[6:], blob[:20]):
        with pytest.raises(Exception) as want:
            container.unpack(bad)
        with pytest.raises(type(want.value)) as got:
            container._index(bad)
        assert str(got.value) == str(want.value)
    # a count no blob can hold: no overflow on the way to the same verdict
    hdr = struct.calcsize("<4sHBBII")
    huge = blob[:hdr + 8] + struct.pack("<Q", (1 << 64) - 1) + blob[hdr + 16:]
    with pytest.raises(ValueError, match="trailing bytes"):
        container._index(huge)
