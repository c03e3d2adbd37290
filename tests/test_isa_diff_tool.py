"""tools/isa_diff.py's kernel-by-kernel comparison (used when a file gained kernels), on
synthetic assembly text: per-file label numbering is ignored, an altered or missing base kernel
is not."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402


def _kernel(name, n, body="\tv_add_f32 v0, v1, v2"):
    return [f"\t.section\t.text.{name},\"axG\",@progbits,{name},comdat",
            f"\t.protected\t{name} ; -- Begin function {name}", f"{name}:", body,
            f".LBB{n}_1:                               ;   in Loop: Header=BB{n}_1 Depth=1",
            f"\ts_cbranch_scc1 .LBB{n}_1", "\ts_endpgm", f"\t.amdhsa_kernel {name}", "\t.end_amdhsa_kernel",
            f".Lfunc_end{n}:", f"\t.size\t{name}, .Lfunc_end{n}-{name}", "                                        ; -- End function",
            "; NumVgprs: 3"]


def _file(kernels):
    lines = []
    for k in kernels:
        lines += k
    lines += ["\t.section\t.AMDGPU.gpr_maximums,\"\",@progbits", "\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for k in kernels:
        name = k[2][:-1]
        lines += ["  - .agpr_count:     0", f"    .name:           {name}", "    .vgpr_count:     3"]
    return lines + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata"]


def test_added_kernel_and_renumbered_labels_are_not_a_difference():
    base = _file([_kernel("_Z1aPf", 0), _kernel("_Z1bPf", 1)])
    new = _file([_kernel("_Z1aPf", 0), _kernel("_Z1cPf", 1), _kernel("_Z1bPf", 2)])
    assert base != new
    assert isa_diff._per_kernel(base, new) == (0, 1)
    assert set(isa_diff._kernels(base)) == {"_Z1aPf", "_Z1bPf"}


def test_altered_or_missing_base_kernel_is_a_difference():
    base = _file([_kernel("_Z1aPf", 0), _kernel("_Z1bPf", 1)])
    altered = _file([_kernel("_Z1aPf", 0), _kernel("_Z1bPf", 1, "\tv_mul_f32 v0, v1, v2"), _kernel("_Z1cPf", 2)])
    assert isa_diff._per_kernel(base, altered) == (1, 1)
    assert isa_diff._per_kernel(base, _file([_kernel("_Z1aPf", 0), _kernel("_Z1cPf", 1)])) == (1, 1)
    meta = [ln.replace("    .vgpr_count:     3", "    .vgpr_count:     4") for ln in base]
    assert isa_diff._per_kernel(base, meta + []) == (2, 0)
