"""Q3_K without a device: the row size, the refusals (each before any device access), a GGUF round trip."""
import numpy as np
import pytest

import ggml_mi355x as g
from tests import gguf_writer, q3k_ref

W, X, Y = 0x10000, 0x20000, 0x30000  # never dereferenced: every status below precedes the launch


def _mul_mat(K, N, M, w=W, nb01=None, q8=False):
    nb01 = K // 256 * 110 if nb01 is None else nb01
    if q8:
        return g.lib().mi355x_mul_mat_q8(g.TYPE_Q3_K, w, K, N, nb01, X, M, K // 256 * 292, Y, N * 4, None)
    return g.lib().mi355x_mul_mat(g.TYPE_Q3_K, w, K, N, nb01, X, M, K * 4, Y, N * 4, None, 0, None)


@pytest.mark.parametrize("q8", [False, True])
def test_mul_mat_refusals(q8):
    assert g.row_size(g.TYPE_Q3_K, 768) == 330
    assert _mul_mat(300, 4, 1, q8=q8) == g.E_INVAL                 # K % 256
    assert _mul_mat(256, 4, 1, w=W + 1, q8=q8) == g.E_INVAL        # an odd address
    assert _mul_mat(256, 4, 1, nb01=111, q8=q8) == g.E_INVAL       # an odd stride
    assert _mul_mat(256, 4, 1, nb01=220, q8=q8) == g.E_UNSUPPORTED  # rows not packed
    assert _mul_mat(256 * 257, 4, 2, q8=q8) == g.E_UNSUPPORTED     # K past the kernel's LDS
    assert q8 or _mul_mat(768, 4, 17) == g.E_WORKSPACE             # 17 columns need their Q8_K rows


def test_fused_entries_and_row_split_refuse_the_type():
    from ggml_mi355x.llama import hparams
    from ggml_mi355x.rowsplit import TokenSplit
    L = g.lib()
    d = (g.GemvDesc * 1)(g.GemvDesc(g.TYPE_Q3_K, W, 4, 110, Y))
    assert L.mi355x_gemv_fused(d, 1, X, 256, None, 0, None) == g.E_UNSUPPORTED
    assert L.mi355x_gemv_fused_ext(d, 1, X, 256, None, None, 0, None) == g.E_UNSUPPORTED
    assert L.mi355x_mul_mat_id(g.TYPE_Q3_K, W, 256, 4, 110, 440, 2, X, 1, 256, Y, 1, 1, 1, Y, None, 0,
                               None) == g.E_UNSUPPORTED
    assert L.mi355x_get_rows(g.TYPE_Q3_K, W, 300, 220, 4, X, 1, Y, None) == g.E_INVAL
    with pytest.raises(g.Mi355xError):
        TokenSplit(hparams(256, 1, 4, 2, 512, 512), 2, 0).slice_weights(
            {"blk.0.attn_q": (g.TYPE_Q3_K, np.zeros((256, 110), np.uint8))})


def test_gguf_round_trip(tmp_path, monkeypatch):
    from ggml_mi355x.gguf import GGUFFile
    monkeypatch.setitem(gguf_writer.TYPE_SIZE, g.TYPE_Q3_K, (256, q3k_ref.BLOCK))
    w = q3k_ref.weights(np.random.default_rng(3), 5, 768)
    gguf_writer.write_gguf(tmp_path / "q3k.gguf", [("general.architecture", gguf_writer.STRING, "llama")],
                           [("blk.0.attn_q.weight", g.TYPE_Q3_K, (768, 5), w.reshape(-1))])
    f = GGUFFile(tmp_path / "q3k.gguf")
    assert f.tensors["blk.0.attn_q.weight"]["type"] == g.TYPE_Q3_K and f.shape_bytes("blk.0.attn_q.weight") == (5, 330)
    assert (f.bytes("blk.0.attn_q.weight") == w.reshape(-1)).all()
    f.close()
