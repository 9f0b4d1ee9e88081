"""The ten kernel-level bench tools at their --quick shapes, in this process: every status assert and every bit comparison a tool makes
holds (main() returns), and its report names every leg of its leg table once per shape.  The four tools that also run a model
(confidence_bench, readings_bench, pronunciation_bench, anchored_loss_bench) are covered by the import test of tests/test_host_benchlib.py
only."""
import importlib
import os
import re
import sys

import pytest

pytestmark = pytest.mark.gpu

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

KERNEL_TOOLS = ("optional_spans_bench", "anchored_bench", "wide_lattice_bench", "repeat_lattice_bench", "dp_ab_bench", "span_confidence_bench",
                "anchored_confidence_bench", "wide_confidence_bench", "repeat_confidence_bench", "song_confidence_bench")


@pytest.mark.parametrize("tool", KERNEL_TOOLS)
def test_quick_run(tool):
    module = importlib.import_module(tool)
    lines = module.main(["--quick"])
    table = module.leg_table(quick=True)
    for name in {name for names in table for name in names}:
        rows = [line for line in lines if re.match(re.escape(name) + r"( +\d+\.\d+ \(\d+\.\d+ \.\. \d+\.\d+\)|$)", line)]   # a table row, or the name alone
        assert len(rows) == sum(name in names for names in table), (name, rows)
