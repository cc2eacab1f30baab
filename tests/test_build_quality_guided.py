"""Static checks on the compiled gfx950 code object of the guided-upsampling kernels (csrc/guided.hip; hipcc cross-compiles, no GPU
needed): every kernel without scratch and without spills, the staged footprint inside one CU's LDS at least twice over, no packed
fp32 arithmetic, and one kernel per (radius, mode) as built."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")


def test_guided_compiles_without_scratch_or_spills_one_kernel_per_radius_and_mode(tmp_path):
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "guided.hip" in SOURCES and SOURCE_FLAGS["guided.hip"] == SOURCE_FLAGS["fullframe.hip"]
    assert "-packed-fp32-ops" in SOURCE_FLAGS["guided.hip"]
    out = tmp_path / "guided.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS["guided.hip"] +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "guided.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    s = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", s, flags=re.M)
    priv = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    spills = re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", s, flags=re.M)
    sspills = re.findall(r"^\s+\.sgpr_spill_count:\s+(\d+)", s, flags=re.M)
    lds = re.findall(r"^\s+\.group_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    assert names and len(priv) == len(names) and len(spills) == len(names) and len(sspills) == len(names) and len(lds) == len(names)
    assert all(int(p) == 0 for p in priv), dict(zip(names, priv))
    assert all(int(p) == 0 for p in spills), dict(zip(names, spills))
    assert all(int(p) == 0 for p in sspills), dict(zip(names, sspills))
    assert all(int(b) <= 80 * 1024 for b in lds), dict(zip(names, lds))   # two blocks per CU (160 KB)
    # guided_kernel<R, MODE>: R = 1, 2, 3 x the four output modes; guided_minmax_kernel<R>: the first launch of DEPTH_RGBA
    main = sorted(n for n in names if "guided_kernel" in n)
    assert len(main) == 12 and len(set(main)) == 12, main
    for radius in (1, 2, 3):
        for mode in (1, 2, 3, 4):
            assert sum(f"guided_kernelILi{radius}ELi{mode}EE" in n for n in main) == 1, (radius, mode, main)
        assert sum(f"guided_minmax_kernelILi{radius}EE" in n for n in names) == 1, (radius, names)
    assert len(names) == 15, names
    assert not re.search(r"v_pk_\w+_f32", s)
