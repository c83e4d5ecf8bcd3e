"""What the folded forward's plan answers, pinned: over the grid of tests/folded_plan_grid.py the library's workspace bytes,
image-contraction passes, side tiles and workgroups per mention equal the answers recorded before the plan existed
(tests/golden/folded_plan_answers.txt, written by tools/folded_plan_answers.py).  A gate or a region size that moves shows up
here as a named row.  Host-only."""
import os

from tests.folded_plan_grid import answers, grid

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "folded_plan_answers.txt")


def test_every_row_of_the_grid_answers_as_recorded():
    with open(GOLDEN) as f:
        want = f.read().split("\n")
    if want[-1] == "":
        want.pop()
    got = answers()
    points = list(grid())
    assert len(got) == len(want) == len(points)
    moved = [(p, w, g) for p, w, g in zip(points, want, got) if w != g]
    assert not moved, "%d rows moved; the first (precision, features, entities, widths, N, T, B), recorded, now: %r" % (len(moved), moved[:5])


def test_the_grid_stands_on_both_sides_of_the_gates():
    """The recorded answers contain every pass count, rows with and without side tiles, and both ends of the chunk rule."""
    with open(GOLDEN) as f:
        rows = [tuple(int(v) for v in line.split()) for line in f.read().split("\n") if line]
    assert {r[1] for r in rows} == {0, 1, 2, 3}
    assert any(r[2] > 0 for r in rows) and any(r[2] == 0 and r[1] in (2, 3) for r in rows)
    assert {1, 7} <= {r[3] for r in rows}             # N = 101 whole (B >= 2048) and in 16-candidate chunks
    assert all(r[0] > 0 and r[0] % 256 == 0 for r in rows)
