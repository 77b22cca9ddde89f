"""Compile-time figures of the kernels (no GPU needed: hipcc cross-compiles gfx950): a unit of lc-crf-slam_amd/csrc compiled with
the library's flags and -Rpass-analysis=kernel-resource-usage, its remarks read per kernel."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _remarks(src):
    """the compiler's resource-usage remarks for one unit, line by line"""
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
           "-I" + os.path.join(ROOT, "lc-crf-slam_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "lc-crf-slam_amd", "csrc", src), "-o", os.devnull]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr.splitlines()


def resource_usage(src):
    """{kernel name: {"VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill": count}}"""
    out, cur = {}, None
    for line in _remarks(src):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def lds_bytes(src):
    """{kernel name: LDS bytes per workgroup} (resource_usage does not read that remark)"""
    out, cur = {}, None
    for line in _remarks(src):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur is not None:
            out[cur] = int(m.group(1))
    return out
