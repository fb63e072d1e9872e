"""Host side of the grouped weight-gradient launch, without a GPU: the tile table ``WgradQueue.tile_table`` builds (XCD
binning, splitting of over-sized problems, -1 padding), the layout of the device image behind the problem array, and the
literal kernel list of tests/test_wgrad_routes_gpu.py against the kernel symbols of the built library.

The kernels' contract is the table: every (problem, n-tile, k-tile) exactly once (a tile listed twice is computed twice --
and under accumulate ADDED twice; a missing one leaves its part of dW unwritten), every other entry -1 in all four fields
(the workgroup returns on .x < 0; the other fields of a padding entry are never read, and stay -1 so that a kernel which
did read them would index far out of any problem rather than silently hit tile 0), a length that keeps blockIdx % 8 = XCD
aligned, and an int4 table that is 16-byte aligned behind the problem array."""
import ctypes
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

KERNEL = re.compile(r"(gemm_bf16_(grouped_)?wgrad\w*kernel|colsum_bf16_kernel|adam(_tiled)?_kernel|ln_bwd(_grouped)?_reduce_kernel)"
                    r"(<[^()]*>)?$")


def _queue():
    from openvivqa_amd import ops
    return ops.WgradQueue


def _check_table(shapes):
    Q = _queue()
    t = Q.tile_table(shapes)
    assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 4
    assert len(t) % 8 == 0 and len(t) > 0
    pad = t[:, 0] < 0
    assert (t[pad] == -1).all(), "a padding entry must be -1 in all four fields"
    real = [tuple(r) for r in t[~pad]]
    want = [(i, c, r, 0) for i, (M, N, K) in enumerate(shapes)
            for c in range(-(-N // Q.TILE)) for r in range(-(-K // Q.TILE))]
    assert len(real) == len(set(real)), "a tile is listed twice"
    assert sorted(real) == sorted(want)
    return t


def _random_shapes(rng, n):
    return [(64 * rng.randint(1, 200), 8 * rng.randint(1, 400), 8 * rng.randint(1, 400)) for _ in range(n)]


@pytest.mark.parametrize("seed", range(8))
def test_every_tile_once_for_random_problem_lists(seed):
    rng = random.Random(seed)
    _check_table(_random_shapes(rng, rng.randint(2, 40)))


def test_single_problem_and_sliver_problems():
    for shapes in ([(6400, 512, 512)], [(64, 8, 8)], [(1, 8, 2048)], [(37, 2048, 8)], [(11648, 5000, 768)]):
        _check_table(shapes)


def test_sixty_one_problems_like_the_mcan_step():
    shapes = []
    for _ in range(6):
        shapes += [(6400, 1536, 512), (6400, 512, 512), (6400, 2048, 512), (6400, 512, 2048)]
    for _ in range(6):
        shapes += [(1280, 1536, 512), (1280, 512, 512), (1280, 2048, 512), (1280, 512, 2048), (6400, 1024, 512),
                   (1280, 512, 512)]
    shapes.append((64, 3000, 1024))
    assert len(shapes) == 61
    _check_table(shapes)


def test_an_oversized_problem_is_split_over_several_xcds():
    """One heavy problem beside a few light ones: n_parts > 1.  Its tiles must then sit in more than one residue class of
    the entry index modulo 8 (the XCD a workgroup lands on), still each exactly once."""
    shapes = [(6400, 1536, 2048), (64, 128, 128), (64, 256, 128), (128, 128, 128)]
    t = _check_table(shapes)
    xcds = {i % 8 for i in range(len(t)) if t[i, 0] == 0}
    assert len(xcds) > 1, xcds
    # whole column blocks (one n-tile with all its k-tiles) of a split problem are not torn across part boundaries more
    # often than the number of parts: every XCD's share of problem 0 is a contiguous run of the (n-tile, k-tile) raster
    for x in xcds:
        mine = [tuple(r[1:3]) for i, r in enumerate(t) if i % 8 == x and r[0] == 0]
        flat = sorted(c * 16 + r for c, r in mine)
        assert flat == list(range(flat[0], flat[0] + len(flat))), (x, mine)


def test_table_image_alignment():
    from openvivqa_amd import _lib
    Q = _queue()
    for n in (1, 2, 3, 61):
        shapes = [(64, 128, 128)] * n
        probs = (_lib.WgradProblem * n)()
        for i in range(n):
            probs[i] = _lib.WgradProblem(0x1000 + i, 0x2000, 0x3000, None, 128, 128, 64, 128, 128, 0)
        tiles = Q.tile_table(shapes)
        for targets in (None, bytes((_lib.AdamTarget * n)())):
            img, tiles_off, targets_off = Q.table_image(bytes(probs), tiles, targets)
            assert tiles_off % 16 == 0 and tiles_off >= ctypes.sizeof(probs) and tiles_off - ctypes.sizeof(probs) < 16
            assert targets_off % 16 == 0 and targets_off >= tiles_off + tiles.nbytes
            assert bytes(img[:ctypes.sizeof(probs)]) == bytes(probs)
            back = np.frombuffer(bytes(img[tiles_off:tiles_off + tiles.nbytes]), dtype=np.int32).reshape(-1, 4)
            assert (back == tiles).all()
            assert len(img) == targets_off + (len(targets) if targets else 0)
            if targets:
                assert bytes(img[targets_off:]) == targets
    assert ctypes.sizeof(_lib.WgradProblem) == 64 and ctypes.sizeof(_lib.AdamTarget) == 48
    assert ctypes.sizeof(_lib.AdamTile) == 32 and ctypes.sizeof(_lib.ReduceProblem) == 40


def _kernel_names(lib_path):
    out = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split(" ", 2)
        if len(parts) < 3 or "__device_stub__" in parts[2]:
            continue
        # (binutils that predate the Itanium mangling of bfloat16, DF16b, leave every symbol with it in a signature mangled)
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", parts[2])
        if m:
            n, rest = int(m.group(1)), parts[2][m.end():]
            name, rest = rest[:n], rest[n:]
            t = re.match(r"I(DF16b|f)E", rest)
            if t:
                name += "<%s>" % {"DF16b": "bf16", "f": "float"}[t.group(1)]
            if KERNEL.match(name):
                names.add(name)
            continue
        sym = parts[2][5:] if parts[2].startswith("void ") else parts[2]
        depth, end = 0, None
        for i, ch in enumerate(sym):  # the name (with its template arguments, if any) ends at the first top-level '('
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0 and not sym.startswith("(anonymous namespace)", i):
                end = i
                break
        if end is None:
            continue
        name = re.sub(r"\(anonymousnamespace\)::|\bovqa::", "", re.sub(r"\s+", "", sym[:end]))
        name = re.sub(r"\b(std::bfloat16_t|__hip_bfloat16|hip_bfloat16|__bf16)\b", "bf16", name)
        if KERNEL.match(name):
            names.add(name)
    return names


def test_wgrad_and_adam_kernel_list_equals_the_library_kernel_symbols():
    from openvivqa_amd import build as B
    import test_wgrad_routes_gpu as R
    if shutil.which("nm") is None:
        pytest.skip("nm (binutils) is not installed: the kernel symbols cannot be listed")
    B.build(verbose=False)
    names = _kernel_names(B.LIB)
    listed = set(R.ALL_KERNELS)
    assert len(listed) == len(R.ALL_KERNELS)
    assert names == listed, {"compiled, in no list": sorted(names - listed), "listed, not compiled": sorted(listed - names)}
