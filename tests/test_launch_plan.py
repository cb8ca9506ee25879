"""pybmc_amd/csrc/bmc_plan.h on the CPU: the launch plan of the Gibbs loop (geometry, kernel
family, how the chains are split over launches) is plain C++ that the library and this test
compile from the same text; here g++ builds tests/launch_plan_check.cpp.

The pinned plans were taken from the planner as it stood before it moved into bmc_plan.h (then
inside run_common), and their kernels from the dispatcher of kernels_gibbs.hip as it stood before
kernel selection moved into bmc_plan.h: a change to any of them changes which kernels a run
launches and has to be measured, not just re-pinned.  Per launch: c0+chains cpp/waves/nslot/pack/
bundle_slots/bundle_bal/resident workgroups=kernel."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

PINNED = """\
ref629x3: vec=1 np=10 | G=1 waves=1 ppg=10 mode=0 ppw=10 nslot=1 cpl=1 one_wave=1 | max=8 passes=1 cpp=1 wpg=1 | 0+1:1/1/1/0/0/0/1=gibbs_wave_kernel<double, 12, 4, 1>
ref629x3_256ch: vec=1 np=10 | G=1 waves=1 ppg=10 mode=0 ppw=10 nslot=256 cpl=256 one_wave=1 | max=256 passes=256 cpp=1 wpg=1 | 0+256:1/1/256/0/0/0/256=gibbs_wave_kernel<double, 12, 4, 1>
ref629x3_f32: vec=1 np=10 | G=1 waves=1 ppg=10 mode=0 ppw=10 nslot=1 cpl=1 one_wave=1 | max=8 passes=1 cpp=1 wpg=1 | 0+1:1/1/1/0/0/0/1=gibbs_wave_kernel<float, 12, 4, 1>
n2500x8_4waves: vec=1 np=40 | G=1 waves=4 ppg=40 mode=0 ppw=10 nslot=1 cpl=1 one_wave=1 | max=8 passes=1 cpp=1 wpg=4 | 0+1:1/4/1/0/0/0/1=gibbs_wave_kernel<double, 12, 8, 4>
n2500x8_256ch: vec=1 np=40 | G=1 waves=4 ppg=40 mode=0 ppw=10 nslot=256 cpl=256 one_wave=1 | max=256 passes=256 cpp=1 wpg=4 | 0+256:1/4/256/0/0/0/256=gibbs_wave_kernel<double, 12, 8, 4>
n8000x4_8waves: vec=1 np=125 | G=1 waves=8 ppg=125 mode=0 ppw=16 nslot=1 cpl=1 one_wave=1 | max=8 passes=1 cpp=1 wpg=8 | 0+1:1/8/1/0/0/0/1=gibbs_wave_kernel<double, 16, 4, 8>
golden64x8: vec=1 np=1 | G=1 waves=1 ppg=1 mode=0 ppw=1 nslot=1 cpl=1 one_wave=1 | max=8 passes=1 cpp=1 wpg=1 | 0+1:1/1/1/0/0/0/1=gibbs_wave_kernel<double, 2, 8, 1>
golden3x2: vec=1 np=1 | G=1 waves=1 ppg=1 mode=0 ppw=1 nslot=1 cpl=1 one_wave=1 | max=8 passes=1 cpp=1 wpg=1 | 0+1:1/1/1/0/0/0/1=gibbs_wave_kernel<double, 2, 4, 1>
c2_1: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=1 one_wave=0 | max=64 passes=1 cpp=1 wpg=5 | 0+1:1/5/8/0/0/0/32=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_1_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=1 one_wave=0 | max=64 passes=1 cpp=1 wpg=5 | 0+1:1/5/8/0/0/0/32=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_8: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=1 wpg=5 | 0+8:1/5/8/0/0/0/256=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_8_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=1 wpg=5 | 0+8:1/5/8/0/0/0/256=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_9: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=9 cpp=1 wpg=5 | 0+8:1/5/8/0/0/0/256=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true> 8+1:1/5/8/0/0/0/32=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_9_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=9 cpp=1 wpg=5 | 0+9:1/5/16/1/0/0/288=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true>
c2_15: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=15 cpp=1 wpg=5 | 0+8:1/5/8/0/0/0/256=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true> 8+7:1/5/8/0/0/0/224=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_15_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=15 cpp=1 wpg=5 | 0+15:1/5/16/1/0/0/480=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true>
c2_16: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=2 wpg=5 | 0+16:2/5/8/0/8/0/256=gibbs_multi_kernel<double, 1, 0, 2, 32, 1, true, false>
c2_16_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=16 cpp=1 wpg=5 | 0+16:1/5/16/1/0/0/512=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true>
c2_32: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=4 wpg=5 | 0+32:4/5/8/0/8/0/256=gibbs_multi_kernel<double, 1, 0, 4, 32, 1, true, false>
c2_32_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=4 wpg=5 | 0+32:4/5/8/0/8/0/256=gibbs_multi_kernel<double, 1, 0, 4, 32, 1, true, false>
c2_40: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=5 cpp=8 wpg=8 | 0+40:8/8/8/0/8/1/160=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true>
c2_40_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=5 cpp=8 wpg=8 | 0+40:8/8/8/0/8/1/160=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true>
c2_63: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=14 cpp=8 wpg=8 | 0+56:8/8/8/0/8/1/224=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true> 56+7:1/5/8/0/0/0/224=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_63_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=14 cpp=8 wpg=8 | 0+56:8/8/8/0/8/1/224=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true> 56+7:1/5/8/0/0/0/224=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_64: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=8 wpg=8 | 0+64:8/8/8/0/8/1/256=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true>
c2_64_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=8 wpg=8 | 0+64:8/8/8/0/8/1/256=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true>
c2_130_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=18 cpp=8 wpg=8 | 0+64:8/8/8/0/8/1/256=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true> 64+64:8/8/8/0/8/1/256=gibbs_multi_kernel<double, 1, 0, 8, 32, 2, true, true> 128+2:1/5/8/0/0/0/64=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_cu128_1: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=4 cpl=1 one_wave=0 | max=32 passes=1 cpp=1 wpg=5 | 0+1:1/5/4/0/0/0/32=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_cu128_16_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=4 cpl=4 one_wave=0 | max=32 passes=4 cpp=4 wpg=5 | 0+16:4/5/4/0/4/0/128=gibbs_multi_kernel<double, 1, 0, 4, 32, 1, true, false>
c2_cu32_1: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=1 wpg=5 | 0+1:1/5/1/0/0/0/32=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_cu32_8: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=8 wpg=8 | 0+8:8/8/1/0/0/0/32=gibbs_multi_kernel<double, 1, 0, 8, 32, 1, false, false>
c4_1: vec=2 np=1563 | G=200 waves=8 ppg=8 mode=0 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=1 wpg=8 | 0+1:1/8/1/0/0/0/200=gibbs_loop_kernel<float, 2, 0, 64, 1, false, false, false>
c4_8: vec=2 np=1563 | G=200 waves=8 ppg=8 mode=0 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=2 cpp=4 wpg=8 | 0+4:4/8/1/0/0/0/200=gibbs_multi_kernel<float, 2, 0, 4, 64, 1, false, false> 4+4:4/8/1/0/0/0/200=gibbs_multi_kernel<float, 2, 0, 4, 64, 1, false, false>
c5_1: vec=1 np=782 | G=200 waves=8 ppg=4 mode=2 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=1 wpg=8 | 0+1:1/8/1/0/0/0/200=gibbs_loop_kernel<double, 1, 2, 0, 0, false, false, false>
c5_8: vec=1 np=782 | G=200 waves=8 ppg=4 mode=2 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=8 wpg=8 | 0+8:8/8/1/0/0/0/200=gibbs_multi_kernel<double, 1, 2, 8, 0, 0, false, false>
hbm410mb_1: vec=4 np=1563 | G=256 waves=8 ppg=7 mode=2 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=1 wpg=8 | 0+1:1/8/1/0/0/0/256=gibbs_loop_kernel<float, 4, 2, 0, 0, false, false, false>
ref629x4_w1: vec=1 np=10 | G=1 waves=1 ppg=10 mode=0 ppw=10 nslot=2 cpl=2 one_wave=1 | max=8 passes=2 cpp=1 wpg=1 | 0+2:1/1/2/0/0/0/2=gibbs_wave_kernel<double, 12, 4, 1>
ref629x4_g10_w1: vec=1 np=10 | G=10 waves=1 ppg=1 mode=0 ppw=1 nslot=8 cpl=2 one_wave=0 | max=8 passes=2 cpp=1 wpg=1 | 0+2:1/1/8/0/0/0/20=gibbs_loop_kernel<double, 1, 0, 8, 1, false, false, true>
n1000x4_g1_w4: vec=1 np=16 | G=1 waves=4 ppg=16 mode=0 ppw=4 nslot=2 cpl=2 one_wave=0 | max=8 passes=2 cpp=1 wpg=4 | 0+2:1/4/2/0/0/0/2=gibbs_loop_kernel<double, 1, 0, 8, 4, true, false, false>
n8000x4_w8: vec=1 np=125 | G=32 waves=8 ppg=4 mode=0 ppw=1 nslot=8 cpl=2 one_wave=0 | max=64 passes=2 cpp=1 wpg=8 | 0+2:1/8/8/0/0/0/64=gibbs_loop_kernel<double, 1, 0, 8, 1, false, false, true>
n3000x8_res3_8ch: vec=1 np=47 | G=12 waves=8 ppg=4 mode=2 ppw=1 nslot=8 cpl=8 one_wave=0 | max=8 passes=1 cpp=8 wpg=8 | 0+8:8/8/8/0/0/0/12=gibbs_multi_kernel<double, 1, 2, 8, 0, 0, false, false>
n3000x8_res3_cpp1: vec=1 np=47 | G=12 waves=8 ppg=4 mode=2 ppw=1 nslot=8 cpl=8 one_wave=0 | max=8 passes=8 cpp=1 wpg=8 | 0+8:1/8/8/0/0/0/96=gibbs_loop_kernel<double, 1, 2, 0, 0, false, false, false>
n3000x8_res2_5ch: vec=1 np=47 | G=12 waves=4 ppg=4 mode=1 ppw=1 nslot=8 cpl=5 one_wave=0 | max=8 passes=2 cpp=4 wpg=4 | 0+4:4/4/8/0/0/0/12=gibbs_multi_kernel<double, 1, 1, 4, 0, 0, false, false> 4+1:1/4/8/0/0/0/12=gibbs_loop_kernel<double, 1, 1, 0, 0, false, false, false>
n700x130_res3_3ch: vec=1 np=11 | G=6 waves=2 ppg=2 mode=2 ppw=1 nslot=8 cpl=3 one_wave=0 | max=8 passes=2 cpp=2 wpg=2 | 0+2:2/2/8/0/0/0/6=gibbs_multi_kernel<double, 1, 2, 2, 0, 0, false, false> 2+1:1/2/8/0/0/0/6=gibbs_loop_kernel<double, 1, 2, 0, 0, false, false, false>
n3000x8_g3_w2_res2: vec=1 np=47 | G=3 waves=2 ppg=16 mode=1 ppw=1 nslot=8 cpl=2 one_wave=0 | max=8 passes=1 cpp=2 wpg=2 | 0+2:2/2/8/0/0/0/3=gibbs_multi_kernel<double, 1, 1, 2, 0, 0, false, false>
c2_19_cpp2_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=11 cpp=2 wpg=5 | 0+16:2/5/8/0/8/0/256=gibbs_multi_kernel<double, 1, 0, 2, 32, 1, true, false> 16+3:1/5/8/0/0/0/96=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_40_cpp4_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=16 cpp=4 wpg=5 | 0+32:4/5/8/0/8/0/256=gibbs_multi_kernel<double, 1, 0, 4, 32, 1, true, false> 32+8:1/5/8/0/0/0/256=gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
c2_64_cpp1_pack: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=16 passes=64 cpp=1 wpg=5 | 0+16:1/5/16/1/0/0/512=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true> 16+16:1/5/16/1/0/0/512=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true> 32+16:1/5/16/1/0/0/512=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true> 48+16:1/5/16/1/0/0/512=gibbs_loop_kernel<double, 1, 0, 32, 1, false, true, true>
c2_64_ppw1: vec=1 np=157 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=8 wpg=8 | 0+64:8/8/8/0/8/0/256=gibbs_multi_kernel<double, 1, 0, 8, 32, 1, true, false>
n9000x16f32_64ch: vec=1 np=141 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=8 wpg=8 | 0+64:8/8/8/0/8/1/256=gibbs_multi_kernel<float, 1, 0, 8, 16, 2, true, true>
n9000x16f32_64ch_ppw1: vec=1 np=141 | G=32 waves=5 ppg=5 mode=0 ppw=1 nslot=8 cpl=8 one_wave=0 | max=64 passes=8 cpp=8 wpg=8 | 0+64:8/8/8/0/8/0/256=gibbs_multi_kernel<float, 1, 0, 8, 16, 1, true, false>
c2_res3_8ch: vec=1 np=157 | G=32 waves=8 ppg=5 mode=2 ppw=1 nslot=8 cpl=8 one_wave=0 | max=8 passes=1 cpp=8 wpg=8 | 0+8:8/8/8/0/0/0/32=gibbs_multi_kernel<double, 1, 2, 8, 0, 0, false, false>
n100000x32_4ch: vec=1 np=1563 | G=200 waves=8 ppg=8 mode=0 ppw=1 nslot=1 cpl=1 one_wave=0 | max=8 passes=1 cpp=4 wpg=8 | 0+4:4/8/1/0/0/0/200=gibbs_multi_kernel<double, 1, 0, 4, 32, 1, false, false>
"""


def _build(tmp_path):
    exe = tmp_path / "launch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", str(exe),
                    os.path.join(HERE, "launch_plan_check.cpp")], check=True)
    return str(exe)


def test_pinned_launch_plans(tmp_path):
    out = subprocess.run([_build(tmp_path)], check=True, capture_output=True, text=True).stdout
    got = dict(line.split(": ", 1) for line in out.splitlines())
    want = dict(line.split(": ", 1) for line in PINNED.splitlines())
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_every_plan_passes_the_launch_checks(tmp_path):
    """Shapes x chain counts x cu_limit x tunings: chains 0..n-1 once and in order, no launch above
    max_per_launch (the exchange words), every launch accepted by launch_gibbs's argument checks and
    running a compiled kernel (kernel_compiled of its key; the simplex geometries too)."""
    res = subprocess.run([_build(tmp_path), "sweep"], capture_output=True, text=True)
    lines = res.stdout.splitlines()
    last = lines[-1].split()
    assert res.returncode == 0 and last[0] == "sweep" and last[2] == "0", res.stdout[-3000:]
    assert int(last[1]) > 1_000_000
    # (which compiled kernels no plan reaches is pinned and asserted by tests/test_kernel_census.py,
    # whose grid contains this sweep's; this line is the sweep's own count)
    print(lines[-2])


def test_kernel_table_matches_the_build(tmp_path):
    """The loop kernels the selection table enumerates (bmc_plan.h, loop_kernel_keys) are exactly
    the kernels hipcc compiled into kernels_gibbs.o (its resource remarks, demangled), apart from
    gibbs_gram_kernel, which has a launcher of its own."""
    res_file = os.path.join(HERE, "..", "pybmc_amd", "csrc", "kernels_gibbs.res")
    if not os.path.exists(res_file):      # (remarks are build products; build() makes them)
        pytest.skip("kernels_gibbs.res not built")
    if shutil.which("c++filt") is None:
        pytest.skip("c++filt not found")
    with open(res_file) as f:
        mangled = re.findall(r"remark: Function Name: (\S+)", f.read())
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True,
                               check=True).stdout.split("\n")
    built = {re.sub(r"^void bmc::(.*)\(bmc::\w+\)$", r"\1", d) for d in demangled if d}
    built = {n for n in built if not n.startswith("gibbs_gram_kernel<")}
    table = subprocess.run([_build(tmp_path), "names"], check=True, capture_output=True, text=True).stdout.split("\n")
    table = [n for n in table if n]
    assert len(table) == len(set(table))
    assert set(table) == built
