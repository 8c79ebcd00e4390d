"""CPU checks of the log-probability path's host side: mi355x_logprob_workspace_size, the order of
mi355x_logprob_rows' argument errors (on fake pointers: all are returned before any device
access), what mi355x_backend_supports_op takes of a LOGPROB_BATCH node, the node list of the
all-rows prompt graph and the refusals of LlamaDecoder.logprobs / .perplexity on a describe-only
decoder. No device, no launch."""
import ctypes

import numpy as np
import pytest

X, TG, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000
ROW = 2176  # the counter's 128-B line + 256 words
V = 32000


def test_workspace_size():
    import ggml_mi355x as g
    for n in (1, 3, 4, 5, 1024, 1025, 32000, 128256, 262144):
        for rows in (1, 2, 3, 8, 512, 65535):
            assert g.logprob_workspace_size(n, rows) == ROW * rows, (n, rows)  # whatever n is
            assert g.logprob_workspace_size(n, rows) == g.argmax_rows_workspace_size(n, rows)  # its layout
    for n, rows in ((0, 1), (-1, 1), (262145, 1), (1 << 24, 1), (32000, 0), (32000, -1), (32000, 65536)):
        assert g.logprob_workspace_size(n, rows) == 0, (n, rows)
        assert g.lib().mi355x_logprob_rows(X, n, rows, max(n, 4) + 4 & ~3, TG, OUT, WS, 1 << 40, None) == g.E_INVAL


def test_argument_errors_in_order_without_device():
    import ggml_mi355x as g
    L = g.lib()
    n, rows = V, 8
    ws = g.logprob_workspace_size(n, rows)

    def call(**kw):
        a = dict(x=X, n=n, rows=rows, stride=n, tg=TG, out=OUT, ws=WS, size=ws)
        a.update(kw)
        return L.mi355x_logprob_rows(a["x"], a["n"], a["rows"], a["stride"], a["tg"], a["out"], a["ws"], a["size"], None)

    bad_args = (dict(x=None), dict(x=X + 4), dict(x=X + 8), dict(stride=n - 4), dict(stride=n + 2),
                dict(n=n - 1, stride=n - 1), dict(n=0), dict(n=262145, stride=262148), dict(rows=0), dict(rows=65536),
                dict(tg=None), dict(tg=TG + 2), dict(out=None), dict(out=OUT + 4))
    for bad in bad_args:
        assert call(**bad) == g.E_INVAL, bad
        # E_INVAL comes before E_WORKSPACE: a bad argument with a bad workspace
        assert call(ws=None, **bad) == g.E_INVAL, bad
        assert call(size=0, **bad) == g.E_INVAL, bad
    for bad in (dict(ws=None), dict(ws=WS + 4), dict(size=ws - 1), dict(size=g.logprob_workspace_size(n, rows - 1))):
        assert call(**bad) == g.E_WORKSPACE, bad
    if not g.device_available():
        assert call() == g.E_NODEVICE
        assert call(n=n - 1, stride=n + 4) == g.E_NODEVICE  # a padded odd row
        assert call(out=OUT + 8) == g.E_NODEVICE            # records are 8-B aligned, not 16


# ---------------------------------------------------------------- supports_op on hand-made nodes
def _node(T, x="ok", tg="ok", dst_type=None, dst_ne0=6, dst_T=None, dst_data=0x9000, n=V):
    import ggml_mi355x as g
    x = g.make_tensor(g.TYPE_F32, n, T, 0x100000) if x == "ok" else x
    tg = g.make_tensor(g.TYPE_I32, T, 1, 0x8000) if tg == "ok" else tg
    return g.make_tensor(g.TYPE_I32 if dst_type is None else dst_type, dst_ne0, T if dst_T is None else dst_T, dst_data,
                         op=g.OP_LOGPROB_BATCH, srcs=[x, tg], flags=g.FLAG_OUTPUT)


@pytest.mark.parametrize("T", [1, 3, 512])
def test_supports_op_accepts(T):
    import ggml_mi355x as g
    assert g.OP_LOGPROB_BATCH == 16
    assert g.supports_op(_node(T))
    for n in (4, 2304, 128256, 262144):
        assert g.supports_op(_node(T, n=n)), n
    assert g.supports_op(_node(T, dst_data=0x9008))  # 8-B aligned records
    assert g.supports_op(_node(65535, n=4))


@pytest.mark.parametrize("T", [1, 3])
def test_supports_op_refuses(T):
    import ggml_mi355x as g
    for n in (V + 1, V + 2, 5, 262148, 1 << 24):                                                  # n % 4, n outside the range
        assert not g.supports_op(_node(T, n=n)), n
    assert not g.supports_op(_node(T, x=g.make_tensor(g.TYPE_F16, V, T, 0x100000)))              # f16 logits
    assert not g.supports_op(_node(T, x=g.make_tensor(g.TYPE_F32, V, T, 0x100004)))              # misaligned
    assert not g.supports_op(_node(T, x=g.make_tensor(g.TYPE_F32, V, T, None)))
    assert not g.supports_op(_node(3, x=g.make_tensor(g.TYPE_F32, V, 3, 0x100000, row_stride=4 * V + 16)))  # strided rows
    strided = g.make_tensor(g.TYPE_F32, V, T, 0x100000)
    strided.nb[0] = 8
    assert not g.supports_op(_node(T, x=strided))
    assert not g.supports_op(_node(T, x=None))
    assert not g.supports_op(_node(65536, n=4))                                                   # T outside the range
    # targets: missing, f32, I64, of another length, no data
    assert not g.supports_op(_node(T, tg=None))
    assert not g.supports_op(_node(T, tg=g.make_tensor(g.TYPE_F32, T, 1, 0x8000)))
    assert not g.supports_op(_node(T, tg=g.make_tensor(g.TYPE_I64, T, 1, 0x8000)))
    assert not g.supports_op(_node(T, tg=g.make_tensor(g.TYPE_I32, T + 1, 1, 0x8000)))
    assert not g.supports_op(_node(T, tg=g.make_tensor(g.TYPE_I32, T, 1, None)))
    # dst: the wrong type, record width, row count, alignment, no data
    assert not g.supports_op(_node(T, dst_type=g.TYPE_F32))
    assert not g.supports_op(_node(T, dst_ne0=5))
    assert not g.supports_op(_node(T, dst_ne0=8))
    assert not g.supports_op(_node(T, dst_T=T + 1))
    assert not g.supports_op(_node(T, dst_data=0x9004))
    assert not g.supports_op(_node(T, dst_data=None))
    # an ARGMAX_BATCH's shape under this op, and the reverse
    as_argmax = _node(T)
    as_argmax.op = g.OP_ARGMAX_BATCH
    assert not g.supports_op(as_argmax)
    plain = g.make_tensor(g.TYPE_I32, T, 1, 0x9000, op=g.OP_LOGPROB_BATCH,
                          srcs=[g.make_tensor(g.TYPE_F32, V, T, 0x100000)], op_params=[g.ARGMAX_PLAIN])
    assert not g.supports_op(plain)


# ---------------------------------------------------------------- the decoder, describe only
@pytest.fixture(scope="module")
def dec():
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_graph_sig as S
    return LlamaDecoder(None, S.HP, S._weights(), S.N_CTX)


def ops(nodes):
    return [n.op for n in nodes]


def test_all_rows_graph_node_list(dec):
    import ggml_mi355x as g
    from tests import llama_graph_sig as S
    n_tok, V_, E = 9, S.HP["n_vocab"], S.HP["n_embd"]
    before = dec._prompt_graph(n_tok)
    sig = [(n.op, tuple(n.ne), n.data, tuple(n.op_params)) for n in before["nodes"]]
    pg = dec._prompt_graph(n_tok, all_rows=True)
    assert pg is not before and dec._prompt_graph(n_tok, all_rows=True) is pg  # a cache entry of its own
    assert dec._prompt_graph(n_tok) is before
    assert [(n.op, tuple(n.ne), n.data, tuple(n.op_params)) for n in before["nodes"]] == sig
    # the prompt graph's ops without the last layer's two GET_ROWS (the row selection), then LOGPROB_BATCH
    want = ops(before["nodes"])
    first = want.index(g.OP_GET_ROWS, 1)
    assert want[first:first + 2] == [g.OP_GET_ROWS, g.OP_GET_ROWS]
    del want[first:first + 2]
    assert ops(pg["nodes"]) == want + [g.OP_LOGPROB_BATCH]
    lp, logits = pg["nodes"][-1], pg["nodes"][-2]
    assert (logits.op, logits.ne[0], logits.ne[1], logits.flags) == (g.OP_MUL_MAT, V_, n_tok, g.FLAG_OUTPUT)
    assert all(n.ne[1] == n_tok for n in pg["nodes"][:-1])  # every row goes through every node and the head
    assert (lp.type, lp.ne[0], lp.ne[1], lp.nb[1], lp.flags) == (g.TYPE_I32, 6, n_tok, 24, g.FLAG_OUTPUT)
    assert lp.data == pg["rec"].data_ptr() and pg["rec"].numel() == 6 * n_tok
    assert ctypes.addressof(lp.src[0].contents) == ctypes.addressof(logits) and not lp.src[2]
    tg = lp.src[1].contents
    assert (tg.type, tg.ne[0], tg.ne[1], tg.data) == (g.TYPE_I32, n_tok, 1, pg["inp"][2 * n_tok:].data_ptr())
    assert pg["inp"].numel() == 3 * n_tok  # token ids | positions | targets
    assert g.supports_op(lp)
    assert pg["logits"].shape == (n_tok, V_) and E == pg["nodes"][0].ne[0]


def test_logprobs_and_perplexity_refusals(dec):
    import ggml_mi355x as g
    from tests import llama_graph_sig as S
    n_ctx, V_ = S.N_CTX, S.HP["n_vocab"]
    toks = list(range(1, 10))
    bad_logprobs = [
        dict(tokens=[]),
        dict(tokens=toks, start_pos=-1),
        dict(tokens=toks, start_pos=n_ctx - 8),             # the last token leaves the cache
        dict(tokens=[1] * (n_ctx + 1)),
        dict(tokens=[1, V_, 2]),                            # a token outside the vocabulary
        dict(tokens=[1, -1, 2]),
        dict(tokens=toks, targets=toks[1:]),                # one target per row
        dict(tokens=toks, targets=toks + [1]),
        dict(tokens=toks, targets=[2 ** 31] + toks[1:]),    # not an int32
    ]
    for kw in bad_logprobs:
        with pytest.raises(g.Mi355xError):
            dec.logprobs(**kw)
    text = [int(t) for t in np.random.default_rng(1).integers(0, V_, 3 * n_ctx)]
    bad_ppl = [
        dict(tokens=text, n_ctx=n_ctx + 1),
        dict(tokens=text, n_ctx=2),
        dict(tokens=text, n_ctx=0),
        dict(tokens=text, n_batch=0),
        dict(tokens=text[:n_ctx - 1]),                      # less than one chunk
        dict(tokens=text, bos=V_),
        dict(tokens=text, bos=-1),
        dict(tokens=[V_] + text[1:]),
    ]
    for kw in bad_ppl:
        with pytest.raises(g.Mi355xError):
            dec.perplexity(**kw)
    dec.split = object()  # a row split
    try:
        with pytest.raises(g.Mi355xError):
            dec.logprobs(toks)
        with pytest.raises(g.Mi355xError):
            dec.perplexity(text)
    finally:
        dec.split = None
    odd = dict(dec.hp, n_vocab=V_ + 2)  # LOGPROB_BATCH's rows are a multiple of 4 entries
    hp, dec.hp = dec.hp, odd
    try:
        with pytest.raises(g.Mi355xError):
            dec.logprobs(toks)
    finally:
        dec.hp = hp
    assert not any(isinstance(k, tuple) and k[1] != 9 for k in dec._prompts)  # refused before a graph was built
