"""Host side of the row-wise kernels (LayerNorm, attention pool, log-softmax, NLL), without a GPU: the literal
instantiation list of tests/test_rowwise_routes_gpu.py against the kernel symbols of the built library, and the Python
copy of the LayerNorm backward's wave / workgroup predicate (csrc/layernorm.hip ``layernorm_bwd_waves`` /
``layernorm_bwd_blocks``) at literal (M, D) pairs on both sides of its two thresholds, M = 4096 and D = 1168.

The symbols are read MANGLED (``nm`` without -C) and their template arguments decoded here: binutils that predate the
Itanium mangling of bfloat16 (DF16b) demangle a kernel with a bf16 argument into nonsense, and every template argument of
these kernels is float, bf16 or an int literal, which five lines decode.  An argument of any other kind stays in the name
undecoded (``pool_fwd_kernel<float,?Lb1EE...>``), so a new kernel of the family is reported by the list test, never dropped."""
import re
import shutil
import subprocess

import pytest

FAMILY = re.compile(r"(ln_fwd_kernel<|ln_bwd_kernel<|pool_fwd_kernel<|pool_bwd_kernel<|log_softmax_(fwd|bwd)(_row)?_kernel<"
                    r"|nll_loss_kernel$)")
SYMBOL = re.compile(r"_ZN(?:4ovqa)?12_GLOBAL__N_1(\d+)")
ARG = re.compile(r"DF16b|f|Li(\d+)E")


def _kernel_names(lib_path):
    """The host-side kernel handles of the anonymous namespaces, as ``_lib.resolve_launch`` writes an instantiation:
    ``ln_bwd_kernel<bf16,float,bf16,2,8>``."""
    out = subprocess.run(["nm", lib_path], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split()
        m = SYMBOL.match(parts[-1]) if parts else None
        if not m:
            continue
        n, rest = int(m.group(1)), parts[-1][m.end():]
        name, rest = rest[:n], rest[n:]
        if name.startswith("__device_stub__"):
            continue
        if rest.startswith("I"):
            args, pos = [], 1
            while rest[pos] != "E":
                a = ARG.match(rest, pos)
                if a is None:  # a template argument of another kind: kept undecoded, so that a kernel of this family
                    args.append("?" + rest[pos:])  # with, say, a bool argument is reported as in no list, not dropped
                    break
                args.append({"DF16b": "bf16", "f": "float"}.get(a.group(0), a.group(1)))
                pos = a.end()
            name += "<%s>" % ",".join(args)
        if FAMILY.match(name):
            names.add(name)
    return names


def test_rowwise_kernel_list_equals_the_library_kernel_symbols():
    from openvivqa_amd import build as B
    import test_rowwise_routes_gpu as R
    if shutil.which("nm") is None:
        pytest.skip("nm (binutils) is not installed: the kernel symbols cannot be listed")
    B.build(verbose=False)
    names = _kernel_names(B.LIB)
    listed = set(R.ALL_ROWWISE)
    assert len(listed) == len(R.ALL_ROWWISE) == 48
    assert names == listed, {"compiled, in no list": sorted(names - listed), "listed, not compiled": sorted(listed - names)}
    count = lambda p: sum(1 for n in names if n.startswith(p))
    assert [count(p) for p in ("ln_fwd_kernel<", "ln_bwd_kernel<", "pool_fwd_kernel<", "pool_bwd_kernel<", "log_softmax_",
                               "nll_loss_kernel")] == [9, 24, 3, 3, 8, 1]


def test_layernorm_bwd_predicate_copy_at_its_thresholds():
    """8 waves need M >= 4096 and 7 * 2 * D * 4 <= 65536 bytes of LDS (D <= 1170, i.e. 1168 among the multiples of 8);
    the workgroup count is ceil(M / waves) capped at 512 (8 waves) or 1024 (4 waves)."""
    from test_rowwise_routes_gpu import ln_bwd_blocks, ln_bwd_waves
    want = {
        (1, 8): (4, 1), (2, 8): (4, 1), (5, 520): (4, 2), (37, 2048): (4, 10),
        (4095, 8): (4, 1024), (4095, 1168): (4, 1024), (4096, 1168): (8, 512), (4096, 1176): (4, 1024),
        (4096, 8): (8, 512), (4088, 8): (4, 1022), (4097, 1176): (4, 1024), (8704, 520): (8, 512), (8704, 1032): (8, 512),
        (9000, 1176): (4, 1024), (9000, 1168): (8, 512), (4096, 2048): (4, 1024), (100000, 1168): (8, 512),
    }
    for (M, D), (waves, blocks) in want.items():
        assert (ln_bwd_waves(M, D), ln_bwd_blocks(M, D)) == (waves, blocks), (M, D)
