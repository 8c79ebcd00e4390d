"""CPU (no launch, no device): which form mi355x_attn_batch takes under mi355x_attn_stream
(mi355x_attn_batch_path; csrc/kq_attn_batch.hip attn_batch_form). Mode 0 keeps today's answers,
mode 1 sends to the streamed form only what kq_attn_batch refuses for its size, mode 2 everything
the streamed kernels take."""
import pytest

TINY = (32, 4, 64)     # n_head, n_head_kv, head_dim
L3_8B = (32, 8, 128)


@pytest.fixture
def stream_mode():
    """Sets mi355x_attn_stream for one test and puts the previous mode back."""
    import ggml_mi355x as g
    prev = []

    def set_mode(mode):
        p = g.attn_stream(mode)
        assert p >= 0
        if not prev:
            prev.append(p)
    yield set_mode
    if prev:
        g.attn_stream(prev[0])


def path(n_ctx, shape, n_kv=None):
    import ggml_mi355x as g
    return g.attn_batch_path(n_ctx, *shape, n_ctx if n_kv is None else n_kv)


def test_the_stream_value_is_no_form_of_kq_attn_batch():
    import ggml_mi355x as g
    assert g.ATTN_PATH_STREAM == 7 and g.ATTN_PATH_STREAM not in (g.ATTN_GROUP, g.ATTN_HEAD)


def test_mode0_refuses_the_sizes_as_before(stream_mode):
    import ggml_mi355x as g
    stream_mode(0)
    assert path(2048, TINY) == g.ATTN_GROUP and path(4096, TINY) == g.ATTN_HEAD  # (8 rows of 4096 cells pass 160 KB)
    assert path(7616, TINY) in (g.ATTN_GROUP, g.ATTN_HEAD) and path(7040, L3_8B) in (g.ATTN_GROUP, g.ATTN_HEAD)
    for n_ctx, shape in ((7648, TINY), (7072, L3_8B), (8224, TINY), (16384, L3_8B), (131072, TINY)):
        assert path(n_ctx, shape) == g.E_UNSUPPORTED, (n_ctx, shape)
    assert path(16384, TINY, 1056) == g.E_UNSUPPORTED  # the cache's size, whatever the row's


def test_mode1_streams_only_what_is_refused_for_its_size(stream_mode):
    import ggml_mi355x as g
    stream_mode(0)
    today = {(n, s): path(n, s) for n in (32, 64, 2048, 4096, 7040) for s in (TINY, L3_8B)}
    stream_mode(1)
    for (n, s), form in today.items():
        assert form in (g.ATTN_GROUP, g.ATTN_HEAD) and path(n, s) == form, (n, s)
    for n_ctx, shape in ((7648, TINY), (7072, L3_8B), (8192, L3_8B), (8224, TINY), (16416, L3_8B), (131072, TINY)):
        assert path(n_ctx, shape) == g.ATTN_PATH_STREAM, (n_ctx, shape)
    assert path(16384, TINY, 1056) == g.ATTN_PATH_STREAM
    # the argument checks are not lifted: n_kv a multiple of 32 inside the cache, n_ctx <= 131072
    assert path(16384, TINY, 1040) == g.E_INVAL and path(16384, TINY, 16416) == g.E_INVAL
    assert path(131072 + 32, TINY) == g.E_UNSUPPORTED


def test_mode2_streams_every_shape_the_kernels_take(stream_mode):
    import ggml_mi355x as g
    stream_mode(2)
    for n_ctx, shape in ((32, TINY), (64, L3_8B), (4096, TINY), (8224, L3_8B), (131072, TINY)):
        assert path(n_ctx, shape) == g.ATTN_PATH_STREAM, (n_ctx, shape)
    assert path(4096, TINY, 96) == g.ATTN_PATH_STREAM
    assert path(4096, TINY, 100) == g.E_INVAL


def test_the_debug_knob_overrides_the_mode(stream_mode):
    import ggml_mi355x as g
    stream_mode(0)
    g.debug_knob("ATTN_STREAM", 1)
    try:
        assert path(8224, TINY) == g.ATTN_PATH_STREAM and path(2048, TINY) == g.ATTN_GROUP
    finally:
        g.debug_knob("ATTN_STREAM")
    assert path(8224, TINY) == g.E_UNSUPPORTED
