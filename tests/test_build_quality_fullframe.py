"""Static checks on the compiled gfx950 code object of the full-frame pre/post kernels (csrc/fullframe.hip; hipcc
cross-compiles, no GPU needed): every kernel without scratch and without spills, and the resize tile inside one CU's LDS
twice over."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")


def test_fullframe_compiles_without_scratch_or_spills(tmp_path):
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "fullframe.hip" in SOURCES and "-packed-fp32-ops" in SOURCE_FLAGS["fullframe.hip"]
    out = tmp_path / "fullframe.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS["fullframe.hip"] +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "fullframe.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    s = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", s, flags=re.M)
    priv = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    spills = re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", s, flags=re.M)
    sspills = re.findall(r"^\s+\.sgpr_spill_count:\s+(\d+)", s, flags=re.M)
    lds = re.findall(r"^\s+\.group_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    for kernel in ("coeff_rect_kernel", "resize_rect_kernel", "post_resize_kernel", "depth_minmax_kernel"):
        assert any(kernel in n for n in names), (kernel, names)
    assert len(priv) == len(names) and len(spills) == len(names) and len(lds) == len(names)
    assert all(int(p) == 0 for p in priv), dict(zip(names, priv))
    assert all(int(p) == 0 for p in spills), dict(zip(names, spills))
    assert all(int(p) == 0 for p in sspills), dict(zip(names, sspills))
    assert all(int(b) <= 80 * 1024 for b in lds), dict(zip(names, lds))   # two blocks per CU (160 KB)
    assert sum("post_resize_kernel" in n for n in names) == 4                # one per output mode
    assert not re.search(r"v_pk_\w+_f32", s)
