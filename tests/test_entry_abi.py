"""CPU check of the decode kernels' entry: the built library's kernel
descriptors give the decode GEMV families a kernarg preload, so their leading plain
parameters are in SGPRs at wave start, and the full 14 dwords the entry is laid out for."""
import os
import re
import shutil
import subprocess

from tests.test_abi import _gfx950_code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# kernel family (mangled-name prefix) -> (the preload length its parameter list is laid out
# for, the fewest kernels of the family the library must hold)
PRELOADED = {
    "_ZN2kq7kq_rowsI": (14, 12),
    "_ZN2kq11kq_rows_dynI": (14, 12),
    "_ZN2kq14kq_attn_decodeI": (14, 8),  # head_dim 64 / 128 x {<=256 cells, batched, 4 slices, 8 slices}
    "_ZN2kq11kq_get_rowsE": (14, 1),
}


def _preload_lengths(path, tmp_path):
    """{kernel: .amdhsa_user_sgpr_kernarg_preload_length} over the library's gfx950 kernels."""
    tool = OBJDUMP if os.path.exists(OBJDUMP) else shutil.which("llvm-objdump")
    assert tool, "llvm-objdump not found"
    out = {}
    for k, obj in enumerate(_gfx950_code_objects(path)):
        p = tmp_path / f"co{k}.o"
        p.write_bytes(obj)
        txt = subprocess.run([tool, "-d", "--mcpu=gfx950", "-j", ".rodata", str(p)], capture_output=True, text=True,
                             check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)\.kd>:", line)
            if m:
                cur = m.group(1)
                out[cur] = 0
                continue
            m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", line)
            if m and cur:
                out[cur] = int(m.group(1))
    return out


def test_decode_kernels_preload_their_leading_parameters(tmp_path):
    import ggml_mi355x as g
    g.lib()
    lengths = _preload_lengths(g.LIB_PATH, tmp_path)
    assert len(lengths) >= 40
    for prefix, (want, members) in PRELOADED.items():
        fam = {n: v for n, v in lengths.items() if n.startswith(prefix)}
        assert len(fam) >= members, (prefix, sorted(fam))
        assert all(v > 0 for v in fam.values()), {n: v for n, v in fam.items() if not v}
        assert all(v == want for v in fam.values()), {n: v for n, v in fam.items() if v != want}
