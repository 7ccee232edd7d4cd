"""Round 10 of the W-in-LDS schedule of the f16-pair forward (rayen_amd/csrc/rayen_mfma_pair_wl.hip), read off the compiler's
output; no GPU needed.  The translation unit is compiled to gfx950 assembly with the flags of rayen_amd/_build.py and the
headline instance <NKK = 2, no arg-max record, one sample tile, sixteen waves, no mapper, screening, no drain> must show

  * the probe reading operands of its own: the conditional overwrite of the walk's A-operand buffer made hipcc copy the
    buffer around, 65 v_mov_b64 in the instance (about 30 executed per probed segment) -- at most 4 are left;
  * no register spilled to scratch and four waves per SIMD, as before;
  * the head in the order the round planned: a wave's first rows -- eight buffer_load_dwordx4 -- requested behind the last
    LDS-DMA of the image and in front of the workgroup barrier, the wait between them leaving exactly those eight in flight.

(Two waves of a workgroup take that path, the others request their rows right behind the barrier: with all sixteen early the
launch was slower, profiles/bench/r10_wl_head_probe.txt.)"""
import os
import re
import subprocess

import pytest

from rayen_amd import _build

HEADLINE = "ILi2ELb0ELi1ELi16ELi0ELb1ELb0EE"      # <2, false, 1, 16, 0, true, false>
SOURCE = "rayen_mfma_pair_wl.hip"


def _assemble(path, defines):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", _build.INCLUDE, "-I", _build.CSRC, *_build.COMMON_FLAGS,
             *_build.EXTRA_FLAGS.get(SOURCE, []), *defines]
    run = subprocess.run([_build.hipcc_path(), *flags, "--cuda-device-only", "-S", os.path.join(_build.CSRC, SOURCE), "-o", path],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    with open(path) as f:
        return f.read()


def _headline(assembly):
    """(instructions of the instance in program-text order, its resource lines, its metadata record)"""
    syms = sorted(set(re.findall(r"^(_ZN5rayen19mfma_pair_wl_kernel" + HEADLINE + r"\w+):", assembly, re.M)))
    assert len(syms) == 1, syms
    sym = syms[0]
    body = re.search(r"^" + re.escape(sym) + r":[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel", assembly, re.S | re.M).group(1)
    ins = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    info = re.search(r"; Kernel info:\n(.*?; Occupancy: \d+)", assembly[assembly.index(sym + ":"):], re.S).group(1)
    meta = re.search(r"\.name:\s+" + re.escape(sym) + r"\n(.*?)\.wavefront_size", assembly, re.S).group(1)
    return ins, info, meta


@pytest.fixture(scope="module")
def headline(tmp_path_factory):
    """The instance as the library builds it."""
    return _headline(_assemble(str(tmp_path_factory.mktemp("pair_wl_isa") / "pair_wl.s"), []))


def _moves(ins):
    return [l for l in ins if l.startswith("v_mov_b64")]


def _resources(info, meta):
    return (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)),
            int(re.search(r"; ScratchSize: (\d+)", info).group(1)), int(re.search(r"; Occupancy: (\d+)", info).group(1)))


def _head(ins):
    """(row loads between the last LDS-DMA of the image and the first barrier, the vmcnt waits behind the last of them)"""
    barrier = next(i for i, l in enumerate(ins) if l.startswith("s_barrier"))
    dmas = [i for i, l in enumerate(ins) if l.startswith("global_load_lds_dwordx4")]
    assert dmas and dmas[-1] < barrier, "the image arrives by LDS-DMA in front of the barrier"
    between = ins[dmas[-1] + 1:barrier]
    at = [i for i, l in enumerate(between) if l.startswith("buffer_load_dwordx4")]
    waits = [l for l in between[(at[-1] + 1 if at else 0):] if l.startswith("s_waitcnt") and "vmcnt" in l]
    return len(at), waits


def test_the_probe_leaves_the_operand_buffer_alone(headline):
    ins, _, _ = headline
    print(f"\n  v_mov_b64 in the headline instance: {len(_moves(ins))} of {len(ins)} instructions")
    assert len(_moves(ins)) <= 4, _moves(ins)


def test_no_spill_and_four_waves_per_simd(headline):
    _, info, meta = headline
    print("\n  " + " | ".join(l.strip("; ") for l in info.split("\n") if re.search(r"NumVgprs|ScratchSize|Occupancy", l)))
    assert _resources(info, meta) == (0, 0, 0, 4)


def test_the_first_rows_are_requested_between_the_image_and_the_barrier(headline):
    ins, _, _ = headline
    loads, waits = _head(ins)
    print(f"\n  between the last LDS-DMA and the barrier: {loads} buffer_load_dwordx4, vmcnt waits behind them {waits}")
    assert loads == 8
    # the wait behind them is for the image alone: the eight rows stay in flight across the barrier
    assert waits and all(re.search(r"vmcnt\((\d+)\)", l).group(1) == "8" for l in waits), waits
