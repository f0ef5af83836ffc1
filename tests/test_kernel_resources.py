"""Register and scratch budget of the kernels of csrc/geometry.hip, csrc/attention.hip and csrc/sampler.hip, read from the compiler's own output (no GPU
needed).

Round 6 folded two opt-in experiments into grid_query_wave_kernel as run-time branches; its default form went from 46 to 100
VGPRs (8 -> 4 waves per SIMD) and nobody saw it, because every A/B compared the switch on with the switch off on the same binary.
This compiles the file to assembly with the flags of csrc/build.py and checks the kernel descriptors, so that it cannot recur
silently.  The attention kernels sit close to occupancy boundaries of their own (168 registers: three waves per SIMD, 256: two);
their budgets are those boundaries."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")


def _build_py():
    spec = importlib.util.spec_from_file_location("npcd_csrc_build", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernels_of(source):
    """Module-scoped fixture: {mangled kernel name: {"vgpr": .amdhsa_next_free_vgpr, "scratch": .amdhsa_private_segment_fixed_size,
    "lds": static bytes}} of one source of csrc/ -- one hipcc run per source for the module."""
    @pytest.fixture(scope="module")
    def fixture(tmp_path_factory):
        return _compile(source, str(tmp_path_factory.mktemp("kernel_resources") / source.replace(".hip", ".s")))
    return fixture


def _compile(source, out):
    build = _build_py()
    if not os.path.exists(build.HIPCC):
        pytest.skip(f"hipcc not found at {build.HIPCC}")
    cmd = [build.HIPCC, *build.COMMON, *build.SOURCES[source], "-S", "--cuda-device-only", os.path.join(CSRC, source), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"hipcc failed:\n{r.stderr}"
    found = {}
    name = None
    keys = {"next_free_vgpr": "vgpr", "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
            continue
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)\s*$", line)
        if m and name:
            found[name][keys[m.group(1)]] = int(m.group(2))
        if ".end_amdhsa_kernel" in line:
            name = None
    assert found, "no kernel descriptor parsed"
    for k, v in found.items():
        assert set(v) == set(keys.values()), (k, v)
        print(f"{k}: {v}")
    return found


kernels = _kernels_of("geometry.hip")
attention = _kernels_of("attention.hip")
sampler = _kernels_of("sampler.hip")


def _form(kernels, name, *flags):
    """The one instantiation name<flags...> (Itanium mangling of bool template arguments: I Lb1E Lb0E ... E)."""
    tag = f"{len(name)}{name}I" + "".join(f"Lb{int(f)}E" for f in flags) + "E"
    hit = [v for k, v in kernels.items() if tag in k]
    assert len(hit) == 1, f"{name}{flags}: {len(hit)} kernels match {tag} in {sorted(kernels)}"
    return hit[0]


def test_no_kernel_of_geometry_uses_scratch(kernels):
    assert len(kernels) >= 17, sorted(kernels)
    spilling = {k: v["scratch"] for k, v in kernels.items() if v["scratch"] != 0}
    assert not spilling, spilling


def test_default_query_forms_keep_eight_waves_per_simd(kernels):
    """51 / 54 VGPRs is what the round-6 source gave with its two experiments compiled out; 56 is the next multiple of the
    8-register allocation granule (a SIMD holds min(8, 512 / allocation) waves: anything up to 64 allows all 8)."""
    for compact in (True, False):
        k = _form(kernels, "grid_query_wave_kernel", compact, False)
        assert k["vgpr"] <= 56, (compact, k)


def test_default_march_forms_do_not_pay_for_the_fused_one(kernels):
    """No more than with the run-time MarchFused argument of round 6 (55 compact, 49 dense)."""
    assert _form(kernels, "ray_march_wave_kernel", True, False)["vgpr"] <= 55
    assert _form(kernels, "ray_march_wave_kernel", False, False)["vgpr"] <= 49


def test_fused_forms_exist(kernels):
    """The opt-in forms are separate instantiations (scratch is checked above; their register counts are not a bar)."""
    _form(kernels, "grid_query_wave_kernel", True, True)
    _form(kernels, "ray_march_wave_kernel", True, True)


def _instances(kernels, name):
    """Every instantiation of the kernel template `name`."""
    return {k: v for k, v in kernels.items() if f"{len(name)}{name}I" in k}


@pytest.mark.parametrize("name,budget", [("attn_fwd_kernel", 168), ("attn_bwd_dq_kernel", 168), ("attn_fwd64_kernel", 256),
                                         ("attn_bwd_dkdv_kernel", 256)])
def test_attention_kernels_keep_their_waves_per_simd(attention, name, budget):
    """A SIMD has 512 registers per lane, allocated in granules of 8: up to 168 allow three waves, up to 256 two.  The 32-row forward
    and the dQ pass run at three (128 against 148 us at two for the forward), the 64-row forward and the dK/dV pass
    are built for two."""
    hit = _instances(attention, name)
    assert len(hit) == 2, (name, sorted(hit))          # bf16 and f16
    for k, v in hit.items():
        assert v["vgpr"] <= budget, (k, v)


def test_attention_scratch(attention):
    """No kernel of the file spills -- except attn_bwd_fused_kernel, the OPT-IN single-pass backward (the training path runs the
    two-pass kernels): it spills 140 bytes per lane and must not get worse."""
    assert len(attention) >= 22, sorted(attention)
    fused = _instances(attention, "attn_bwd_fused_kernel")
    assert len(fused) == 2, sorted(fused)
    for k, v in fused.items():
        assert v["scratch"] <= 140, (k, v)
    spilling = {k: v["scratch"] for k, v in attention.items() if v["scratch"] != 0 and k not in fused}
    assert not spilling, spilling


def test_attention_forward_has_no_shelved_forms(attention):
    """The 32-row forward exists once per element type (no row-split instantiation beside it), and the forward with K / V resident
    in LDS is gone (docs/experiments.md R11.1 has both as patches)."""
    assert len(_instances(attention, "attn_fwd_kernel")) == 2, sorted(attention)
    assert not [k for k in attention if "attn_fwd_res" in k], sorted(attention)


def test_sampler_kernels_keep_eight_waves_per_simd_without_scratch(sampler):
    """One kernel template stands behind the three entries of the scheduled step (no masks and no history, masks, masks and history);
    written as three separate kernels they took 24 / 32 / 38 VGPRs.  64 is the most that still allows all 8 waves per SIMD: below
    it the occupancy of these streaming kernels cannot change.  No kernel of the file spills."""
    steps = _instances(sampler, "sampler_step_kernel")
    assert len(steps) == 3 and len(_instances(sampler, "ddpm_reverse_kernel")) == 2, sorted(sampler)
    for masks, hist in ((False, False), (True, False), (True, True)):
        k = _form(sampler, "sampler_step_kernel", masks, hist)
        print(f"sampler_step_kernel<masks={masks}, hist={hist}>: {k}")
        assert k["vgpr"] <= 64, (masks, hist, k)
    spilling = {k: v["scratch"] for k, v in sampler.items() if v["scratch"] != 0}
    assert not spilling, spilling
