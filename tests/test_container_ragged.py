"""The container's per-stream n_symbols for streams of different lengths (host only)."""
import pytest

from lac_amd import container


def test_pack_unpack_unequal_n_symbols():
    streams = [b"", b"\x80", bytes(range(9)), b"\xff\x00"]
    n_symbols = [0, 1, 130, 17]
    n_bits = [0, 1, 70, 9]
    blob = container.pack(streams, n_symbols, n_bits, prec=40, vocab=1000)
    h = container.unpack(blob)
    assert h["n_symbols"] == n_symbols and h["n_bits"] == n_bits and h["streams"] == streams
    assert (h["prec"], h["vocab"], h["pmf_bits"], h["q1_logits"]) == (40, 1000, 32, False)


def test_compress_batch_takes_n_symbols():
    """The new argument is part of the signature and validated before any encode."""
    import inspect
    assert "n_symbols" in inspect.signature(container.compress_batch).parameters

    class _Coder:
        streams = 2

    class _Sym:
        shape = (5, 2)

    torch = pytest.importorskip("torch")
    pmf = torch.zeros((5, 2, 4), dtype=torch.int32)
    for bad in ([1, 2, 3], [1, 6], [-1, 2]):
        with pytest.raises(ValueError):
            container.compress_batch(_Coder(), pmf, _Sym(), n_symbols=bad)
