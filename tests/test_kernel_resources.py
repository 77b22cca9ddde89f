"""Compile-time guard for the two hand-tuned kernels (no GPU needed: hipcc cross-compiles gfx950).

The one-workgroup-per-frame kernels' SLAM variants must not spill: scratch traffic inside the
mean-field loop costs more than any optimisation in those files gains, and
chain_rows' hand-written ring relies on v96..v127 being free around it.  The fused build must not
spill vector registers either."""
import re
import shutil

import pytest

from kernel_resources import HIPCC, resource_usage


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_fused_slam_variants_do_not_spill():
    """Every BASELINE configuration's variant -- 1000 / 2000 keypoints (1-2 points per lane) and 3000 (3 points per lane,
    config C4) -- runs without scratch memory."""
    use = resource_usage("fused_engine.hip")
    fused = {k: v for k, v in use.items() if "k_fusedI" in k}
    # 1024 lanes: PPT 1..4 x K 1..2 x {short rows, chain}; 512 lanes: PPT 1..2 x ...; each x MODE {0 self-contained, 1 prepare, 2 from
    # the prepared launch records (round 6)}
    assert len(fused) == 72
    for name, r in fused.items():
        nt, ppt, mode = (int(x) for x in re.search(r"k_fusedILi(\d+)ELi(\d)ELi\dELi\dELi(\d)E", name).groups())
        assert nt in (512, 1024) and mode in (0, 1, 2)
        # 128 registers per lane: 1024 lanes fill the CU's register file; two 512-lane workgroups (small frames) share it
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, name
        if ppt <= 3:
            assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_two_full_size_frames_per_cu_fit_the_register_file_without_scratch():
    """Round 5 (csrc/fused_lean.h): frames of 513 .. 2048 keypoints as 512-lane workgroups, 2 to 4 points per lane, TWO workgroups per
    CU -- which only works at 128 registers per lane (four wavefronts per SIMD) and only pays without scratch traffic in the loop.
    The rings of the ordered row sums clobber v96..v127; what must survive them passes through the asm statements as operands."""
    use = resource_usage("fused_engine.hip")
    lean = {k: v for k, v in use.items() if "k_fused_leanI" in k}
    # PPT 1..4 x K 1..2 x {short rows, chain} (PPT <= 2: everything in registers) x MODE {0 self-contained, 1 prepare, 2 from the
    # prepared launch records (round 6)}
    assert len(lean) == 48
    for name, r in lean.items():
        nt, ppt, mode = (int(x) for x in re.search(r"k_fused_leanILi(\d+)ELi(\d)ELi\dELi\dELb\dELi(\d)E", name).groups())
        assert nt == 512 and ppt in (1, 2, 3, 4) and mode in (0, 1, 2)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, name
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_frame_kernel_slam_variants_do_not_spill():
    """The one-launch-per-frame kernel: no scratch up to 3 points per lane (C1-C4; VERDICT r2 item 7: the 3-points-per-lane
    shape used to spill 56 bytes per lane in its build phases), nor for 4 points per lane with one kernel."""
    use = resource_usage("frame_engine.hip")
    frame = {k: v for k, v in use.items() if "k_frame" in k}
    assert len(frame) == 16                                   # 1024 lanes: PPT 1..4 x K 1..2; 512 lanes: PPT 1..2 x K 1..2; two-workgroup form: PPT 1..4
    for name, r in frame.items():
        nt, ppt, K, dual = (int(x) for x in re.search(r"k_frameILi(\d+)ELi(\d)ELi(\d)ELb(\d)E", name).groups())
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, name
        if dual:                                              # single frames: a few spilled registers in the 2-points-per-lane shape
            assert r["ScratchSize [bytes/lane]"] <= (32 if ppt <= 3 else 160), (name, r)
        elif ppt <= 3 or K == 1:
            assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        else:
            assert r["ScratchSize [bytes/lane]"] <= 160, (name, r)      # 4 points per lane, two kernels (3073-4096 points): 132 B


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_half_cu_frame_kernel_has_no_scratch_and_no_scalar_spills():
    """Round 5 (csrc/frame_lean.hip): lattice build + normalisation + inference of a frame in 512 lanes on half a CU, 1 to 4 points
    per lane.  128 registers per lane (two workgroups per CU), no scratch -- and no SCALAR spills either: one spilled scalar register
    reserves a vector register for the whole kernel, which the loop at 4 points per lane does not have (the late kernel-argument
    reads and the scalar plan of that file exist for this)."""
    use = resource_usage("frame_lean.hip")
    lean = {k: v for k, v in use.items() if "k_frame_leanI" in k}
    assert len(lean) == 4                                     # PPT 1..4
    for name, r in lean.items():
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, name
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_fused_build_does_not_spill_vector_registers():
    use = resource_usage("build_small.hip")
    build = {k: v for k, v in use.items() if "k_build_small" in k}
    assert len(build) == 3                                    # d = 1, 2, 3
    for name, r in build.items():
        assert r["VGPRs Spill"] == 0 and r["VGPRs"] <= 128, (name, r)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_streaming_iteration_kernels_use_no_scratch():
    """The streaming engine's iteration kernels are small; scratch there is an accident, not a trade -- round 4 met one:
    `ok ? lds[i] : zero` on float2 selects between two ADDRESSES and parks the zero in scratch (16 B per lane, the splat window 2 x
    slower).  Every splat / blur / slice / softmax variant of the engine's three units must compile without it."""
    units = [resource_usage("stream_%s.hip" % u) for u in ("build", "filter", "pointwise")]
    use = {k: v for unit in units for k, v in unit.items()}
    assert len(use) == sum(len(unit) for unit in units) == 144      # every kernel of the engine, each in one unit only
    it = {k: v for k, v in use.items() if re.search(r"k_(splat|blur|slice|softmax|map|nbr_compact|row_|long_rows)", k)}
    assert len(it) == 53                                      # (k_blur2c has one form: its table is never loaded non-temporally)
    for name, r in it.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
