"""The rule of mi355x_penalize_rows (include/ggml_mi355x.h) restated in numpy float32, one operation
per rounding: the sampler's repetition / frequency / presence penalties over a window of past
tokens and a logit bias, in place on a row of logits. The device gives the same bits.

Row i of x is edited from its window, the history entries hist[i][j] for the j with
end[i] - last_n < j <= end[i] and 0 <= j < n_hist, and the bias list. A token id outside [0, n)
(unsigned compare) is ignored, in the window and in the list. For a token t with c(t) window
entries and the bias entries B(t) (in list order); untouched if c(t) == 0 and B(t) is empty:
  1. v = x[t]
  2. for each k in B(t), in order: v = v + bias_val[k]
  3. if c(t) > 0: v = (v <= 0) ? v * repeat : v / repeat; v = v - ((float)c(t) * freq + present)
  4. x[t] = v
"""
import numpy as np

F = np.float32
MAX_LAST_N, MAX_BIAS = 1024, 256


def window(hist_row, end, last_n):
    """The window of one row: the entries j of hist_row with end - last_n < j <= end (Python ints:
    no overflow at the int32 extremes)."""
    end, n_hist = int(end), len(hist_row)
    lo, hi = max(end - int(last_n) + 1, 0), min(end, n_hist - 1)
    return [int(t) for t in hist_row[lo:hi + 1]] if last_n > 0 and hi >= lo else []


def penalize_row(x, win=(), repeat=1.0, freq=0.0, present=0.0, bias=()):
    """The rule on one row: (the edited copy of x, the mask of the entries it wrote). win: the
    window's token ids; bias: (token, value) pairs in list order, or a dict {token: value}."""
    x = np.array(x, dtype=F)
    bias = bias.items() if isinstance(bias, dict) else bias
    n = x.shape[0]
    repeat, freq, present = F(repeat), F(freq), F(present)
    count, biases = {}, {}
    for t in win:
        if 0 <= int(t) < n:
            count[int(t)] = count.get(int(t), 0) + 1
    for t, b in bias:
        if 0 <= int(t) < n:
            biases.setdefault(int(t), []).append(F(b))
    touched = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for t in sorted(set(count) | set(biases)):
            v = x[t]
            for b in biases.get(t, ()):
                v = F(v + b)
            c = count.get(t, 0)
            if c > 0:
                v = F(v * repeat) if v <= 0 else F(v / repeat)
                cost = F(F(F(c) * freq) + present)
                v = F(v - cost)
            x[t] = v
            touched[t] = True
    return x, touched


def penalize_rows(x, hist=None, end=None, last_n=0, repeat=1.0, freq=0.0, present=0.0, bias=(), n=None):
    """The rule on every row of the matrix x [rows, >= n] (n None: the whole row; the columns from n
    on are padding and stay): (the edited copy, the mask of written entries). hist [rows, n_hist],
    end [rows]."""
    x = np.array(x, dtype=F)
    if x.ndim == 1:
        x = x[None, :]
    n = x.shape[1] if n is None else n
    touched = np.zeros(x.shape, dtype=bool)
    for i in range(x.shape[0]):
        win = window(np.asarray(hist)[i], np.asarray(end)[i], last_n) if last_n > 0 else []
        x[i, :n], touched[i, :n] = penalize_row(x[i, :n], win, repeat, freq, present, bias)
    return x, touched


def same(got, want, touched):
    """Equal as uint32, except that an entry the rule wrote may hold any NaN where the reference
    holds one (the rule: "a NaN logit stays NaN"; which NaN an operation returns is the
    hardware's)."""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    eq = got.view(np.uint32) == want.view(np.uint32)
    return bool((eq | (touched & np.isnan(got) & np.isnan(want))).all())


def first_mismatch(got, want, touched):
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    eq = (got.view(np.uint32) == want.view(np.uint32)) | (touched & np.isnan(got) & np.isnan(want))
    bad = np.argwhere(~eq)
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return f"{len(bad)} entries differ, first at {i}: got {got[i]!r} ({got.view(np.uint32)[i]:#x}), " \
           f"want {want[i]!r} ({want.view(np.uint32)[i]:#x})"
