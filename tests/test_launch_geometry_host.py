"""The launch-geometry helpers of rayen_amd/csrc/rayen_launch_geometry.h (persistent_grid, grid_for_groups, rows_aligned16) give
the integers the launchers used to compute in place (no GPU).

A small host-only C++ program includes the header, evaluates the helpers over a grid of (batch, rows per group, SIMD
count, waves per SIMD, waves per workgroup) and prints the results; the expected values are computed here, in Python
integers, with the formula as every launcher spelled it out before the helpers existed:

    n_groups = ceil(B / per_wave); rounds = ceil(n_groups / slots); waves = ceil(n_groups / rounds);
    grid = ceil(waves / block_waves)

Exact equality.  ``launch_simds()``, through which the reserved CUs enter, stays outside the helpers: the SIMD counts
below stand for its result."""
import itertools
import shutil
import subprocess

from rayen_amd import _build

BATCHES = [1, 31, 32, 33, 500, 4096, 32768, 65536, 98304, 131072, 262144, 524288, 1048576, 2 ** 31 + 5]
PER_WAVE = [32, 64]
SIMDS = [4, 992, 1024]
# (slots per SIMD as a fraction num / den, waves per workgroup): two waves per SIMD in workgroups of eight (the tile
# walks) and of four (the fp64 kernels' order of size), and one workgroup per CU (the W-stationary kernel)
SHAPES = [(2, 1, 8), (2, 1, 4), (1, 4, 1)]


def _ceil(a, b):
    return -(-a // b)


def _parent_grid(B, per_wave, slots, block_waves):
    n_groups = _ceil(B, per_wave)
    rounds = _ceil(n_groups, slots)
    waves = _ceil(n_groups, rounds)
    return n_groups, _ceil(waves, block_waves)


def _cases():
    for B, per_wave, simds, (num, den, block) in itertools.product(BATCHES, PER_WAVE, SIMDS, SHAPES):
        yield B, per_wave, simds * num // den, block


def test_geometry_helpers_match_the_written_out_formula(tmp_path):
    rows = ",\n".join(f"  {{{B}ll, {pw}, {slots}ll, {block}}}" for B, pw, slots, block in _cases())
    src = tmp_path / "geometry_probe.cpp"
    src.write_text(f"""
#include <cstdio>
#include "rayen_launch_geometry.h"
struct Case {{ long long B; int per_wave; long long slots; int block_waves; }};
static const Case cases[] = {{
{rows}
}};
int main() {{
  for (const Case& c : cases) {{
    const long long n_groups = (c.B + c.per_wave - 1) / c.per_wave;
    std::printf("%lld %lld %lld\\n", n_groups,
                (long long)rayen::grid_for_groups(n_groups, c.slots, c.block_waves),
                (long long)rayen::persistent_grid(c.B, c.per_wave, c.slots, c.block_waves));
  }}
  alignas(16) static float buf[12];
  std::printf("%d %d %d %d %d\\n", (int)rayen::rows_aligned16(buf, 4), (int)rayen::rows_aligned16(buf, 6),
              (int)rayen::rows_aligned16(buf + 1, 4), (int)rayen::rows_aligned16(buf + 4, 8),
              (int)rayen::base_aligned16(buf + 2));
  return 0;
}}
""")
    exe = tmp_path / "geometry_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    cmd = [gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    lines = ran.stdout.strip().splitlines()
    cases = list(_cases())
    assert len(lines) == len(cases) + 1
    for line, (B, per_wave, slots, block) in zip(lines, cases):
        n_groups, grid = _parent_grid(B, per_wave, slots, block)
        got = [int(x) for x in line.split()]
        print(B, per_wave, slots, block, "->", got)
        assert got == [n_groups, grid, grid], (B, per_wave, slots, block, got, (n_groups, grid))
    assert lines[-1].split() == ["1", "0", "0", "1", "0"]
