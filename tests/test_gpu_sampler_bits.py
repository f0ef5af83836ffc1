"""The step kernels of the scheduled sampler (csrc/sampler.hip) give the bits of the commit before they became one kernel template:
tests/golden/sampler_bits_parent.json is the output of tools/sampler_bits.py on that commit's build (three separate kernels in
csrc/elementwise.hip, every loop written out per entry, mode and access width), on an MI355X.  The cases cover the three entries over
eps type, clip, noise, the mode pairs, masks on none / one / both tensors, the 16-byte and the one-element path and the 16-byte loop
past the grid cap; operands are drawn on the CPU from seeded generators and the tables are made on the host, so the digests depend
neither on a library nor on the machine (docs/experiments.md R29.1)."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def test_every_output_has_the_bits_of_the_parent_commit():
    spec = importlib.util.spec_from_file_location("npcd_sampler_bits", os.path.join(ROOT, "tools", "sampler_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(GOLDEN, "sampler_bits_parent.json")) as f:
        parent = json.load(f)
    seen, differing = set(), []
    for case in tool.cases():
        for what, out in tool.run(case, tool.operands(case[2], case[3], case[7])).items():
            key = f"{case[0]}/{what}"
            seen.add(key)
            if tool.digest(out) != parent[key]:
                differing.append(key)
    assert seen == set(parent), sorted(seen ^ set(parent))
    assert not differing, differing
