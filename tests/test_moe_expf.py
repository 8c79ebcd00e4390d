"""kq_moe_route's libm_expf (csrc/kq_moe.hip) restated on the host, against the expf of this host's libm.

The router's soft_max takes the entries beyond n_expert & ~3 through libm's expf [U] (with 2 experts both
entries). The rule's restatement (oracle.kq_ops_oracle.soft_max_row) calls the host's libm; the device carries
glibc's algorithm: exp2f_data's 32-entry table and cubic in double, with the fused multiply-adds of the build
that CPUs with FMA dispatch to. So the bit-exactness of such rows holds where the host's expf is that build:
this test is where the dependence shows. The table and the constants are read from the kernel's source, the
arithmetic is restated with libm's double fma. On a host whose expf is glibc's unfused build a handful of
arguments in 2^31 differ by one ulp; the test names them."""
import ctypes
import ctypes.util
import os
import re
import struct

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ggml-neon-opt_amd", "csrc", "kq_moe.hip")
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.argtypes, _libm.expf.restype = [ctypes.c_float], ctypes.c_float
_libm.fma.argtypes, _libm.fma.restype = [ctypes.c_double] * 3, ctypes.c_double


def _source_constants():
    src = open(SRC).read()
    tab = re.search(r"kExp2fTab\[32\] = \{(.*?)\};", src, re.S).group(1)
    table = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{16})ull", tab)]
    assert len(table) == 32
    body = src[src.index("float libm_expf(float x)"):]
    hexf = lambda name: float.fromhex(re.search(name + r" = (0x[0-9a-fp.+-]+)", body).group(1))  # noqa: E731
    return table, hexf("kInvLn2N") * 32.0, hexf("C0") / 32.0 ** 3, hexf("C1") / 32.0 ** 2, hexf("C2") / 32.0


def _bits64(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def device_expf(x, table, inv_ln2n, c0, c1, c2):
    """libm_expf's arithmetic, operation for operation (Python floats are doubles; fma is libm's)."""
    x = float(np.float32(x))
    if x < float.fromhex("-0x1.9fe368p6"):
        return np.float32(0.0)
    if x > float.fromhex("0x1.62e42ep6"):
        return np.float32(np.inf)
    shift = float.fromhex("0x1.8p+52")
    z = inv_ln2n * x
    kd = z + shift
    ki = _bits64(kd)
    kd -= shift
    r = z - kd
    s = struct.unpack("<d", struct.pack("<Q", (table[ki % 32] + (ki << 47)) & (2 ** 64 - 1)))[0]
    z = _libm.fma(c0, r, c1)
    y = _libm.fma(c2, r, 1.0)
    y = _libm.fma(z, r * r, y)
    return np.float32(y * s)


def test_table_is_two_to_the_i_over_32():
    table = _source_constants()[0]
    for i, t in enumerate(table):
        v = struct.unpack("<d", struct.pack("<Q", t + (i << 47)))[0]
        assert abs(v - 2.0 ** (i / 32.0)) <= 2.0 ** -52 * v, i


def test_device_expf_is_the_hosts_expf():
    consts = _source_constants()
    rng = np.random.default_rng(0xE)
    xs = np.concatenate([
        -np.exp(rng.uniform(np.log(1e-6), np.log(104.0), 60000)),        # the soft_max tail's domain: x <= 0
        -rng.uniform(80.0, 104.5, 5000),                                  # denormal results and the underflow edge
        np.array([0.0, -0.0, -1e-45, -87.3, -87.33655, -88.0, -103.0, -103.27893, -103.97, -104.0, -1e30, -np.inf]),
        rng.uniform(0.0, 88.7, 2000)]).astype(np.float32)
    bad = []
    for x in xs:
        want = np.float32(_libm.expf(float(x)))
        got = device_expf(x, *consts)
        if want.view(np.uint32) != got.view(np.uint32):
            bad.append((float(x).hex(), float(want).hex(), float(got).hex()))
    assert not bad, bad[:8]
