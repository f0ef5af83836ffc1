"""Register and scratch budget of the weight-gradient kernels of csrc/gemm.hip, read from the compiler's own output (no GPU needed).

wgrad_kernel and wgrad_group_kernel run one 512-thread workgroup per CU on 160 KiB of LDS: two waves per SIMD, i.e. at most 256
registers per lane, and nothing in scratch -- the 64-token pipeline of the tile body (docs/experiments.md R21.1) keeps two fragment sets
and eight 32 x 32 accumulators in registers (197 / 198 when it landed; 195 / 196 before it), and a spill would put scratch traffic
into a loop that is paced by its matrix instructions."""
import pytest

from test_kernel_resources import _compile, _instances


@pytest.fixture(scope="module")
def gemm(tmp_path_factory):
    return _compile("gemm.hip", str(tmp_path_factory.mktemp("wgrad_resources") / "gemm.s"))


@pytest.mark.parametrize("name", ["wgrad_kernel", "wgrad_group_kernel"])
def test_weight_gradient_kernels_keep_two_waves_per_simd_and_no_scratch(gemm, name):
    hit = _instances(gemm, name)
    assert len(hit) == 2, (name, sorted(gemm))          # bf16 and f16
    for k, v in hit.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 256, (k, v)
