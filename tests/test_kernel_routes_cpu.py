"""The literal instantiation lists of tests/test_kernel_routes_gpu.py against the kernels the built library contains.

ALL_INSTANTIATIONS (what the route table must reach) and UNREACHABLE_INSTANTIATIONS (compiled, never launched, each with the
predicate that excludes it in that module's docstring) together must be exactly the MFMA GEMM and attention kernel
instantiations whose host-side symbols ``nm -C`` finds in libovqa_hip.so: a new kernel form without a route row, or a row
list that drifts from the source, fails here without a GPU."""
import re
import shutil
import subprocess

import pytest

KERNEL = re.compile(r"(gemm_bf16_(glds_|skinny_)?kernel|ovqa_t256::kernel|attn_\w+_mfma_kernel)<")


def _kernel_names(lib_path):
    out = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split(" ", 2)
        if len(parts) < 3 or not parts[2].startswith("void "):
            continue
        sym, depth, end = parts[2][5:], 0, None
        for i, ch in enumerate(sym):  # the name with its template arguments ends at the '(' after the closing '>'
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0 and i > 0 and sym[i - 1] == ">":
                end = i
                break
        if end is None:
            continue
        name = re.sub(r"\(anonymousnamespace\)::|\bovqa::", "", re.sub(r"\s+", "", sym[:end]))  # as _lib.resolve_launch
        if KERNEL.match(name):
            names.add(name)
    return names


def test_route_lists_equal_the_library_kernel_symbols():
    from openvivqa_amd import build as B
    import test_kernel_routes_gpu as R
    if shutil.which("nm") is None:
        pytest.skip("nm (binutils) is not installed: the kernel symbols cannot be listed")
    B.build(verbose=False)
    names = _kernel_names(B.LIB)
    listed = set(R.ALL_INSTANTIATIONS) | set(R.UNREACHABLE_INSTANTIATIONS)
    assert not set(R.ALL_INSTANTIATIONS) & set(R.UNREACHABLE_INSTANTIATIONS)
    assert names == listed, {"compiled, in no list": sorted(names - listed), "listed, not compiled": sorted(listed - names)}
