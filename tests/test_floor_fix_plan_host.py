"""The ticket layout of the one-launch floor fix-up of the n_fft = 1024 one-pass gate (noisereduce_amd/csrc/onepass_plan.hpp:
floor_fix_plan; onepass.hpp: k_floor_fix) on the host: blocks per unit, the boundary between the maxima tickets and the tile
tickets, and a grid that holds both ranges.  tests/floor_fix_plan_host.cpp is a stand-alone program around the header's function
(built with the host compiler, -fsanitize=address,undefined where the compiler has them).

Every frame of every unit must lie in exactly one maxima block of its unit (16 frames per block: k_stft_bits<512, 4, 4>), every
maxima ticket must be lower than every tile ticket (the wait's progress argument rests on it), and every tile ticket of the first
launch must appear once.  Shapes: the units x tiles of tests/test_gpu_floor_one_launch.py (5 and 10 units of 21 / 37 frames,
2 / 3 tiles + 2 halo tiles) plus the benchmark's 48 units x 149 tiles (2579 frames), one unit of one frame, and counts that do
not fit 32 bits (ok == false: the caller keeps the two launches)."""
import os
import subprocess

import pytest

from tests.test_onepass_plan_host import CXX, ROOT


SRC = os.path.join(ROOT, "tests", "floor_fix_plan_host.cpp")
FRAMES = 16


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    assert CXX is not None
    exe = str(tmp_path_factory.mktemp("floor_fix_plan") / "floor_fix_plan_host")
    base = [CXX, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizer runtimes)
        subprocess.run(base, check=True)
    return exe


def _run(prog, units, T, tiles):
    out = subprocess.run([prog, str(units), str(T), str(tiles)], check=True, capture_output=True, text=True).stdout.split("\n")
    blocks, n_max, grid, ok = (int(v) for v in out[0].split())
    return blocks, n_max, grid, bool(ok), [tuple(int(v) for v in line.split()) for line in out[1:] if line]


@pytest.mark.parametrize("units, T, n_tiles", [(5, 21, 2), (5, 37, 3), (10, 21, 2), (10, 37, 3), (48, 2579, 147), (1, 1, 1),
                                               (3, 16, 2), (3, 17, 2)])
def test_layout(prog, units, T, n_tiles):
    tiles = units * (n_tiles + 2)
    blocks, n_max, grid, ok, tickets = _run(prog, units, T, tiles)
    assert ok
    assert blocks == -(-T // FRAMES) and n_max == units * blocks
    assert grid >= n_max and grid >= tiles and grid == n_max + tiles, "one workgroup per ticket of both ranges"
    assert len(tickets) == grid
    # maxima tickets: all below the boundary, unit-major, every frame of every unit in exactly one block
    covered = {}
    for tk, (role, u, idx) in enumerate(tickets):
        assert (role == 0) == (tk < n_max), "ticket %d: every maxima ticket is lower than every tile ticket" % tk
        if role == 0:
            assert 0 <= u < units and 0 <= idx < blocks
            for t in range(idx * FRAMES, min(T, (idx + 1) * FRAMES)):
                assert (u, t) not in covered
                covered[(u, t)] = tk
    assert len(covered) == units * T
    assert sum(1 for r, _, _ in tickets if r == 0) == units * blocks, "the arrival word of a unit counts to `blocks`"
    # tile tickets: the first launch's tickets 0 .. tiles - 1, once each, in order
    assert [idx for r, _, idx in tickets if r == 1] == list(range(tiles))


def test_the_benchmark_shape_is_48_by_149(prog):
    """10 minutes at 48 kHz in chunks of 600000 + 2 x 30000: 48 units of 2579 frames, 147 tiles + 2 halo tiles."""
    blocks, n_max, grid, ok, _ = _run(prog, 48, 2579, 48 * 149)
    assert ok and blocks == 162 and n_max == 48 * 162 and grid == 48 * 162 + 7152


@pytest.mark.parametrize("units, T, tiles", [(0, 21, 20), (5, 0, 20), (5, 21, 0), (1 << 20, 1 << 20, 5), (4, 16, (1 << 31) - 3),
                                             (1 << 31, 16, 8)])
def test_counts_that_do_not_fit(prog, units, T, tiles):
    blocks, n_max, grid, ok, tickets = _run(prog, units, T, tiles)
    assert not ok and not tickets and (blocks, n_max, grid) == (0, 0, 0)


def test_the_largest_counts_that_fit(prog):
    blocks, n_max, grid, ok, _ = _run(prog, 4, 16, (1 << 31) - 1 - 4)
    assert ok and grid == (1 << 31) - 1
