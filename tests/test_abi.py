"""CPU checks of the C-ABI library: it loads, exports every symbol the header
declares, and its host-side logic (sizes, argument validation, supports_op)
behaves — without launching anything."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ggml_mi355x.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mi355x_[a-z0-9_A-Z]+)\s*\(", src)))


def test_header_symbols_exported():
    import ggml_mi355x as g
    g.lib()
    names = header_functions()
    assert len(names) >= 20
    assert sorted(g.EXPORTED_SYMBOLS) == names
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    missing = [n for n in names if n not in exported]
    assert not missing, missing


def test_library_is_gfx950_code_object():
    import ggml_mi355x as g
    blob = open(g.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for other in (b"--gfx942", b"--gfx90a", b"--gfx1100"):
        assert other not in blob
    assert "gfx950" in g.version()


def test_row_sizes():
    import ggml_mi355x as g
    assert g.row_size(g.TYPE_Q4_K, 2048) == 8 * 144
    assert g.row_size(g.TYPE_Q5_K, 2048) == 8 * 176
    assert g.row_size(g.TYPE_Q6_K, 5632) == 22 * 210
    assert g.row_size(g.TYPE_Q8_K, 4096) == 16 * 292
    assert g.row_size(g.TYPE_Q4_K, 100) == 0


def test_argument_validation_without_device():
    import ggml_mi355x as g
    L = g.lib()
    # K not a multiple of 256
    assert L.mi355x_mul_mat(12, 0x1000, 300, 4, 144, 0x2000, 1, 1200, 0x3000, 16, None, 0, None) == -1
    # unsupported src0 type
    assert L.mi355x_mul_mat(2, 0x1000, 256, 4, 144, 0x2000, 1, 1024, 0x3000, 16, None, 0, None) == -2
    # empty shapes are a no-op success
    assert L.mi355x_mul_mat(12, 0x1000, 256, 0, 144, 0x2000, 1, 1024, 0x3000, 16, None, 0, None) == 0
    assert L.mi355x_mul_mat(12, 0x1000, 256, 4, 144, 0x2000, 0, 1024, 0x3000, 16, None, 0, None) == 0
    # M > 1 needs a workspace
    assert L.mi355x_mul_mat(12, 0x1000, 256, 4, 144, 0x2000, 3, 1024, 0x3000, 16, None, 0, None) == -3
    assert L.mi355x_mul_mat_workspace_size(12, 2048, 64, 5) == ((5 * 8 * 304 + 255) // 256) * 256
    assert L.mi355x_mul_mat_workspace_size(12, 2048, 64, 1) == 0
    assert L.mi355x_mul_mat_workspace_size(12, 28672, 64, 1) == ((112 * 304 + 255) // 256) * 256
    # the f16 prefill image is sized only once mi355x_prefill_precision selects it
    exact = L.mi355x_mul_mat_workspace_size(12, 4096, 14336, 512)
    assert exact == ((512 * 16 * 304 + 255) // 256) * 256
    prev = L.mi355x_prefill_precision(g.PREFILL_F16)
    try:
        assert L.mi355x_mul_mat_workspace_size(12, 4096, 14336, 512) > exact
    finally:
        L.mi355x_prefill_precision(prev)
    assert L.mi355x_mul_mat_workspace_size(12, 4096, 14336, 512) == exact
    # misaligned weights
    descs = (g.GemvDesc * 1)(g.GemvDesc(12, 0x1002, 4, 144, 0x3000))
    assert L.mi355x_gemv_fused(descs, 1, 0x2000, 256, None, 0, None) == -1
    # row stride too small
    descs = (g.GemvDesc * 1)(g.GemvDesc(12, 0x1000, 4, 100, 0x3000))
    assert L.mi355x_gemv_fused(descs, 1, 0x2000, 256, None, 0, None) == -1
    # large K needs the Q8_K workspace
    assert L.mi355x_gemv_fused_workspace_size(2048) == 0
    assert L.mi355x_gemv_fused_workspace_size(14336) == ((56 * 304 + 255) // 256) * 256
    descs = (g.GemvDesc * 1)(g.GemvDesc(12, 0x1000, 4, 56 * 144, 0x3000))
    prev = L.mi355x_gemv_impl(1)  # kq_gemv quantizes K > 8192 into the workspace
    try:
        assert L.mi355x_gemv_fused(descs, 1, 0x2000, 14336, None, 0, None) == -3
    finally:
        L.mi355x_gemv_impl(prev)
    assert L.mi355x_gemv_impl(7) == -1
    prev = L.mi355x_gemv_impl(2)  # GEMV_ROWS
    assert L.mi355x_gemv_impl(prev) == 2
    prev = L.mi355x_gemv_impl(3)  # GEMV_DYN (claimed rows)
    assert L.mi355x_gemv_impl(prev) == 3
    assert L.mi355x_gemv_impl(4) == -1
    # the prefill tile selector takes 0..4 and 6; 5 (the retired TILE128X) is refused like any
    # other value and leaves the selector as it was
    prev = L.mi355x_mmq_impl(3)  # MMQ_TILE128W
    try:
        for bad in (5, 7, -1):
            assert L.mi355x_mmq_impl(bad) == -1  # MI355X_E_INVAL
        assert L.mi355x_mmq_impl(3) == 3
    finally:
        L.mi355x_mmq_impl(prev)
    # no device here -> the HIP path reports it instead of falling back
    descs = (g.GemvDesc * 1)(g.GemvDesc(12, 0x1000, 4, 144, 0x3000))
    rc = L.mi355x_gemv_fused(descs, 1, 0x2000, 256, None, 0, None)
    assert rc == (0 if g.device_available() else -4)


def test_supports_op():
    import ggml_mi355x as g
    g.lib()
    K, N, M = 2048, 64, 1
    w = g.make_tensor(g.TYPE_Q4_K, K, N, 0x1000)
    x = g.make_tensor(g.TYPE_F32, K, M, 0x2000)
    y = g.make_tensor(g.TYPE_F32, N, M, 0x3000, op=g.OP_MUL_MAT, src0=w, src1=x)
    assert g.supports_op(y)
    for bad_type in (0, 2, 8, 15):
        wb = g.make_tensor(bad_type, K, N, 0x1000)
        assert not g.supports_op(g.make_tensor(g.TYPE_F32, N, M, 0x3000, op=g.OP_MUL_MAT, src0=wb, src1=x))
    xb = g.make_tensor(g.TYPE_F32, K + 256, M, 0x2000)
    assert not g.supports_op(g.make_tensor(g.TYPE_F32, N, M, 0x3000, op=g.OP_MUL_MAT, src0=w, src1=xb))
    w3 = g.make_tensor(g.TYPE_Q6_K, K, N, 0x1000)
    w3.ne[2] = 2
    assert not g.supports_op(g.make_tensor(g.TYPE_F32, N, M, 0x3000, op=g.OP_MUL_MAT, src0=w3, src1=x))


def test_product_has_no_oracle_dependency():
    """The shipped package must not import or link the oracle."""
    pkg = os.path.join(ROOT, "ggml-neon-opt_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                assert "kq_oracle" not in txt and "oracle/" not in txt, fn
    out = subprocess.run(["ldd", os.path.join(pkg, "lib", "libggml_mi355x.so")], capture_output=True, text=True)
    assert "oracle" not in out.stdout


def test_product_reads_no_environment():
    """no run-time environment switch in the product. The library's sources
    have no getenv and the shared library imports none; A/B knobs go through the explicit
    mi355x_debug_knob() entry point and hold the product defaults until set; precision
    changes only through mi355x_prefill_precision()."""
    import ggml_mi355x as g
    src = os.path.join(ROOT, "ggml-neon-opt_amd", "csrc")
    for fn in sorted(os.listdir(src)):
        txt = open(os.path.join(src, fn), errors="ignore").read()
        assert "getenv" not in txt and "secure_getenv" not in txt, fn
    out = subprocess.run(["nm", "-D", "--undefined-only", g.LIB_PATH], capture_output=True, text=True).stdout
    assert not [l for l in out.splitlines() if "getenv" in l], out
    L = g.lib()
    os.environ["MI355X_PREFILL"] = "f16"  # the old switch: no effect any more
    try:
        assert g.prefill_precision(-1) == g.PREFILL_EXACT
    finally:
        del os.environ["MI355X_PREFILL"]
    for k in g.DEBUG_KNOBS:
        d = g.debug_knob(k, 5)  # the default in force before
        assert g.debug_knob(k) == 5  # NaN: restore the default ...
        assert g.debug_knob(k) == d  # ... which is what it then reads
    assert g.debug_knob("GEMV_PRE0") == 1 and g.debug_knob("GEMV_FQMAX") == 144
    prev = __import__("ctypes").c_double(0)
    assert L.mi355x_debug_knob(b"NO_SUCH_KNOB", 1.0, None) == -1
    assert L.mi355x_debug_knob(None, 1.0, prev) == -1


def _gfx950_code_objects(path):
    """gfx950 ELF code objects of every clang offload bundle in the shared library."""
    import struct
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    objs, i = [], data.find(magic)
    while i >= 0:
        n = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(n):
            eo, es, tl = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + tl].decode(errors="replace")
            off += tl
            if "gfx950" in triple and es:
                objs.append(data[i + eo:i + eo + es])
        i = data.find(magic, i + 1)
    return objs


def test_kernels_do_not_spill_to_scratch(tmp_path):
    """A scratch spill in a GEMV costs a vmcnt(0) drain of the weight ring per use
    (seen once: -30 % tok/s). Every kernel must have private_segment_fixed_size 0."""
    import re
    import shutil
    import subprocess
    import ggml_mi355x as g
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    objs = _gfx950_code_objects(g.LIB_PATH)
    assert objs, "no gfx950 code object in the library"
    kernels = 0
    for k, obj in enumerate(objs):
        p = tmp_path / f"co{k}.o"
        p.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        names = re.findall(r"\.name:\s+(\S+)", notes)
        sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
        assert len(names) == len(sizes)
        spilled = [n for n, sz in zip(names, sizes) if sz]
        assert not spilled, f"kernels using scratch: {spilled}"
        kernels += len(names)
    assert kernels >= 20


# Register budgets of the hot kernels (VGPRs incl. AGPRs, from the code object). kq_rows
# runs 12 waves per workgroup = 3 per SIMD (<= 168 registers); the prefill budgets sit a
# little above today's counts: round 2 found timing diagnostics compiled in as run-time
# branches (kq_mmq<Q4_K> 152 -> 192, kq_mmq<Q5_K> 244 -> 368 registers) costing 40 % of
# the 8B ffn_up GEMM. Raising a budget needs a measurement.
VGPR_BUDGET = [
    (r"^_ZN2kq7kq_rows", 168),
    (r"^_ZN2kq6kq_mmqILi12ELi(64|128)ELi1E", 160),
    (r"^_ZN2kq6kq_mmqILi13ELi(64|128)ELi1E", 256),
    (r"^_ZN2kq6kq_mmqILi14ELi(64|128)ELi1E", 168),
    # the wide tiles (two MFMA column tiles per wave): 128 x 128 is one 8-wave workgroup per
    # CU by LDS, two waves per SIMD, so the budget is 256; 64 x 128 one 4-wave workgroup,
    # one wave per SIMD (512, no spill)
    (r"^_ZN2kq6kq_mmqILi1[2-4]ELi128ELi2E", 256),
    (r"^_ZN2kq6kq_mmqILi1[2-4]ELi64ELi2E", 512),
    (r"^_ZN2kq14kq_attn_decode", 256),
]


def test_hot_kernel_register_budgets(tmp_path):
    import re
    import shutil
    import subprocess
    import ggml_mi355x as g
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    seen = {pat: 0 for pat, _ in VGPR_BUDGET}
    over = []
    for k, obj in enumerate(_gfx950_code_objects(g.LIB_PATH)):
        p = tmp_path / f"co{k}.o"
        p.write_bytes(obj)
        notes = subprocess.run([readelf, "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        names = re.findall(r"\.name:\s+(\S+)", notes)
        vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
        spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)]
        assert len(names) == len(vgprs) == len(spills)
        for n, v, sp in zip(names, vgprs, spills):
            for pat, budget in VGPR_BUDGET:
                if re.match(pat, n):
                    seen[pat] += 1
                    # a spill can also move the destination of an in-flight inline-asm load
                    # (the weight prefetches), not only cost time
                    if v > budget or sp:
                        over.append((n, v, budget, sp))
    assert all(seen.values()), f"budgeted kernels missing: {[p for p, c in seen.items() if not c]}"
    assert not over, f"kernels over their register budget: {over}"


# ------------------------------------------------ ISA lint: in-flight load destinations
def _lint():
    import importlib.util
    spec = importlib.util.spec_from_file_location("vmem_lint", os.path.join(ROOT, "tools", "vmem_lint.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_vmem_lint_product_library_clean():
    """No kernel of the product library names a VGPR of a vector-memory load while the
    load can be in flight (tools/vmem_lint.py: the in-order vmcnt model over every path of
    the kernel's control flow). This is the invariant the inline-asm activation loads of
    kq_rows / kq_gemv rely on (round 2's aperture fault came from breaking it)."""
    import ggml_mi355x as g
    res = _lint().lint_library(g.LIB_PATH)
    assert len(res) >= 40
    bad = {k: v[:3] for k, v in res.items() if v}
    assert not bad, bad


def _compile_device(tmp_path, src_text=None, src_file=None, defines=()):
    import subprocess
    out = tmp_path / "co.o"
    src = src_file
    if src_text is not None:
        src = tmp_path / "k.hip"
        src.write_text(src_text)
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", f"-I{ROOT}/include", f"-I{ROOT}/ggml-neon-opt_amd/csrc",
           "--cuda-device-only", "-c", str(src), "-o", str(out)] + [f"-D{d}" for d in defines]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_vmem_lint_flags_a_missing_wait(tmp_path):
    """The lint is not vacuous: a kernel that uses an inline-asm load's register without a
    covering s_waitcnt is flagged, the same kernel with the wait is clean, and kq_rows
    built with its activation wait removed (KQ_ROWS_LINT_BREAK, never run) is flagged."""
    L = _lint()
    src = r'''
#include <hip/hip_runtime.h>
extern "C" __global__ void k(const float *p, float *o) {
    float r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p + threadIdx.x) : "memory");
    %WAIT%
    o[threadIdx.x] = r * 2.0f;
}
'''
    for wait, expect in (("", True), ('asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); asm volatile("" : "+v"(r));',
                                      False)):
        co = _compile_device(tmp_path, src_text=src.replace("%WAIT%", wait))
        hz = [h for obj in L.code_objects(str(co)) for n, ins in L.disassemble(obj).items()
              for h in L.lint_kernel(n, ins)]
        assert bool(hz) == expect, (wait, hz)
    co = _compile_device(tmp_path, src_file=os.path.join(ROOT, "ggml-neon-opt_amd/csrc/kq_rows.hip"),
                         defines=("KQ_ROWS_LINT_BREAK=1",))
    flagged = {n for obj in L.code_objects(str(co)) for n, ins in L.disassemble(obj).items()
               if "kq_rows" in n and L.lint_kernel(n, ins)}
    assert any("ELb1E" in n for n in flagged), flagged  # the fused-quantization (asm-load) kernels
