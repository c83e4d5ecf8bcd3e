"""Prints what the library answers over the grid of tests/folded_plan_grid.py - workspace bytes, image-contraction passes, side
tiles, workgroups per mention, one line per configuration in grid order.  Host-only, under a second.

    python tools/folded_plan_answers.py > tests/golden/folded_plan_answers.txt

regenerates the file tests/test_folded_plan_host.py compares against.  Do that ONLY from a library built from the commit whose
answers are meant to stand (DRIN_LIB_PATH selects it); a change that moves a row has to say why."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests.folded_plan_grid import answers  # noqa: E402

if __name__ == "__main__":
    print("\n".join(answers()))
