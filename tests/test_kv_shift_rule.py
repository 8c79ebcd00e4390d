"""tests/kv_shift_ref.py against itself: the properties of mi355x_kv_shift's rule that the GPU tests
rely on (CPU only)."""
import numpy as np
import pytest

from tests import kv_shift_ref as K

N_POS = 48


def table_of(head_dim, n_pos=N_POS):
    """A rope table [n_pos, head_dim / 2, 2] (cos, sin) of float32; the rule takes any table."""
    i = np.arange(head_dim // 2, dtype=np.float64)
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * 10000.0 ** (-2.0 * i / head_dim)[None, :]
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)


def caches(seed, n_ctx, head_dim, n_head_kv=2):
    rng = np.random.default_rng(seed)
    kvw = n_head_kv * head_dim
    return K.random_cache(rng, (n_ctx, kvw)), K.random_cache(rng, (kvw, n_ctx))


def test_fmaf_rounds_once():
    """A case where the float64 product path rounds twice: 1 + 2^-24 + 2^-60 is above the tie."""
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    exact = K.fmaf(a, b, c)  # 1 + 2^-11 + 2^-24 + 2^-60 -> rounds up
    twice = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert exact == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and twice == np.float32(1 + 2.0 ** -11)
    assert K.fmaf(np.float32(3), np.float32(5), np.float32(-7)) == np.float32(8)


@pytest.mark.parametrize("hd", [64, 128])
def test_delta_zero_is_the_identity(hd):
    k, _ = caches(1, 8, hd)
    k[3, :4] = [0x7c00, 0xfc00, 0x7e01, 0xfdff]  # not rewritten: non-finite values keep their bits too
    assert (K.shift_deltas(k, np.zeros(8, np.int32), table_of(hd), hd) == k).all()
    assert (K.shift_row(k[3], 0, table_of(hd), hd) == k[3]).all()


@pytest.mark.parametrize("hd", [64, 128])
def test_plus_and_minus_use_one_row_with_the_sine_negated(hd):
    k, _ = caches(2, 4, hd)
    tab = table_of(hd)
    d = 17
    neg = tab.copy()
    neg[d, :, 1] = -neg[d, :, 1]
    assert (K.shift_row(k[1], -d, tab, hd) == K.shift_row(k[1], d, neg, hd)).all()
    assert not (K.shift_row(k[1], -d, tab, hd) == K.shift_row(k[1], d, tab, hd)).all()
    # one pair by hand
    x0, x1 = (np.array([k[1, 2 * 5], k[1, 2 * 5 + 1]], np.uint16).view(np.float16).astype(np.float32))
    c, s = tab[d, 5]
    want = np.array([K.fmaf(x0, c, -(x1 * s)), K.fmaf(x0, s, x1 * c)], np.float32).astype(np.float16).view(np.uint16)
    assert (K.shift_row(k[1], d, tab, hd)[10:12] == want.ravel()).all()
    # every head takes the same pair index: channel 2i of head 1 uses table entry i
    assert (K.shift_row(k[1], d, tab, hd)[hd:] == K.shift_row(np.concatenate([k[1, hd:], k[1, hd:]]), d, tab, hd)[:hd]).all()


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("keep,discard,n_past", [(0, 1, 40), (5, 3, 33), (0, 20, 40), (17, 22, 40), (4, 36, 40), (7, 9, 16)])
def test_discard_is_gather_then_deltas(hd, keep, discard, n_past):
    n_ctx = 40
    k, v = caches(3, n_ctx, hd)
    tab = table_of(hd)
    k1, v1 = K.shift_discard(k, v, tab, hd, keep, discard, n_past)
    end = n_past - discard
    gathered = k.copy()
    gathered[keep:end] = k[keep + discard:n_past]
    delta = np.zeros(n_ctx, np.int32)
    delta[keep:end] = -discard
    assert (k1 == K.shift_deltas(gathered, delta, tab, hd)).all()
    for ch in (0, hd - 1, 2 * hd - 1):
        assert (v1[ch, keep:end] == v[ch, keep + discard:n_past]).all()
    # cells outside [keep, n_past - discard) keep their bits
    assert (k1[:keep] == k[:keep]).all() and (k1[end:] == k[end:]).all()
    assert (v1[:, :keep] == v[:, :keep]).all() and (v1[:, end:] == v[:, end:]).all()
    if end > keep:
        assert not (k1[keep:end] == k[keep:end]).all()
    else:
        assert (k1 == k).all() and (v1 == v).all()
    assert (k == caches(3, n_ctx, hd)[0]).all()  # the inputs are copies' sources: untouched


def test_an_out_of_table_delta_gives_nan_bits():
    hd = 64
    k, _ = caches(4, 6, hd)
    tab = table_of(hd)
    delta = np.array([0, N_POS - 1, N_POS, -N_POS, -(N_POS - 1), -2 ** 31], np.int64)
    out = K.shift_deltas(k, delta, tab, hd)
    assert (out[0] == k[0]).all()
    for c in (2, 3, 5):
        assert (out[c] == K.NAN_BITS).all() and np.isnan(out[c].view(np.float16)).all()
    for c in (1, 4):
        assert not np.isnan(out[c].view(np.float16)).any()
