"""The planner's side of the staggered two-slice launch (kernel-id bits 27-28, w4a16_plan.hip shape_xw): host-only, no GPU.

The plan text gains ONE word, `stagger=<d>`, between `xcd_rows=` and `workspace=`, and only for launches that take the variant; every forced id
without the bits describes exactly what it described before the variant existed (the texts below were printed by the library of the commit
before it)."""
import pytest

XW = 5
XW128x128x2 = XW | (4 << 4) | (2 << 8) | (1 << 12)

BEFORE = {
    ((512, 4096, 4096), 0x5): "xw tokens=128 channels=256 waves=4 ring=4 queue=4 grid=256 slices=4 xcd_rows=1 workspace=16842752",
    ((512, 4096, 4096), 0x1245): "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2 xcd_rows=1 workspace=16842752",
    ((512, 4096, 4096), 0x245): "xw tokens=128 channels=256 waves=4 ring=4 queue=4 grid=128 slices=2 xcd_rows=1 workspace=16842752",
    ((512, 4096, 4096), 0x1445): "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2 xcd_rows=1 workspace=16842752",
    ((512, 4096, 4096), 0x225): "xw tokens=64 channels=128 waves=4 ring=8 queue=8 grid=256 slices=1 xcd_rows=2 workspace=0",
    ((512, 4096, 4096), 0x2001245): "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2 xcd_rows=1 workspace=16842752",
    ((512, 4096, 4096), 0x85): "xw tokens=256 channels=256 waves=4 ring=2 queue=2 grid=32 slices=1 xcd_rows=2 workspace=0",
    ((512, 11008, 4096), 0x1245): "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2 xcd_rows=1 workspace=16842752",
    ((512, 11008, 4096), 0x245): "xw tokens=128 channels=256 waves=4 ring=4 queue=4 grid=128 slices=2 xcd_rows=1 workspace=16842752",
    ((300, 4096, 4096), 0x1245): "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=192 slices=2 xcd_rows=1 workspace=16842752",
    ((300, 4096, 4096), 0x225): "xw tokens=64 channels=128 waves=4 ring=8 queue=8 grid=160 slices=1 xcd_rows=1 workspace=0",
    ((1024, 4096, 4096), 0x5): "xw tokens=128 channels=256 waves=4 ring=4 queue=4 grid=256 slices=2 xcd_rows=2 workspace=16842752",
    ((1024, 4096, 4096), 0x1245): "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=1 xcd_rows=2 workspace=0",
    ((1024, 4096, 4096), 0x85): "xw tokens=256 channels=256 waves=4 ring=2 queue=2 grid=64 slices=1 xcd_rows=2 workspace=0",
}


def test_the_staggered_loop_is_what_the_generator_writes(tmp_path):
    """quick_amd/csrc/w4a16_xws_loop.inc is checked in like the other generated loops: byte for byte what tools/gen_xw_loop.py writes today.  The
    generator asserts hazard distances and counted waits, and that each use of the one parametrised statement (product, phase stamps, gate
    experiment) is string for string the statement it builds for that use."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_xw_loop", os.path.join(root, "tools", "gen_xw_loop.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.staggered_file() == open(os.path.join(root, "quick_amd", "csrc", "w4a16_xws_loop.inc")).read()
    assert [c.name for c in gen.STAGGERED] == ["41s"]


@pytest.fixture(scope="module")
def describe():
    from quick_amd import kernels
    return kernels.plan_describe


def test_forced_ids_without_the_bits_describe_what_they_did_before(describe):
    for ((M, K, N), kid), text in BEFORE.items():
        assert describe(M, K, N, 128, kid) == text, ((M, K, N), hex(kid))


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_stagger_word_sits_between_xcd_rows_and_workspace(describe, d):
    for M, K, N in ((512, 4096, 4096), (512, 11008, 4096), (300, 4096, 4096), (509, 4096, 4096)):
        plain = describe(M, K, N, 128, XW128x128x2)
        text = describe(M, K, N, 128, XW128x128x2 | (d << 27))
        head, ws = plain.rsplit(" ", 1)
        assert ws.startswith("workspace=") and text == f"{head} stagger={d} {ws}"
        assert text.startswith("xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=") and " slices=2 " in text
        assert text.split()[0] == "xw" and text.split()[-1] == ws           # (family from the first word, workspace= the last)
    assert describe(512, 4096, 4096, 128, XW128x128x2 | (d << 27)).startswith(
        "xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2")


def test_a_stagger_the_variant_cannot_run_is_planned_without_it(describe):
    S2 = 2 << 27
    for (M, K, N, G), kid in (((512, 1024, 4096, 128), XW128x128x2 | (1 << 27)),      # phase 1 of 3 stages: shorter than the ring
                              ((512, 1280, 4096, 128), XW128x128x2 | S2),
                              ((512, 4224, 4096, 128), XW128x128x2 | S2),              # 33 k tiles: the slices are not equal
                              ((512, 4096, 4096, 256), XW128x128x2 | S2),              # group size
                              ((512, 4096, 4096, 128), XW | (4 << 4) | (2 << 8) | S2),  # 128 x 256 tiles
                              ((256, 4096, 4096, 128), XW | (4 << 4) | (4 << 8) | (1 << 12) | S2),   # four slices
                              ((512, 4096, 4096, 128), XW | (4 << 4) | (1 << 8) | (1 << 12) | S2),   # one slice
                              ((1024, 4096, 4096, 128), XW128x128x2 | S2),             # 256 tiles: one slice each
                              ((513, 4096, 4096, 128), XW128x128x2 | S2),              # 160 tiles: one slice each
                              ((256, 4096, 4096, 128), XW | (2 << 4) | (2 << 8) | S2),  # 64 x 128 tiles
                              ((512, 4096, 4096, 128), XW | (8 << 4) | S2)):           # 256 x 256 tiles
        text = describe(M, K, N, G, kid)
        assert "stagger" not in text and text == describe(M, K, N, G, kid & ~(3 << 27)), ((M, K, N, G), hex(kid))
    assert " stagger=3 " in describe(512, 1792, 4096, 128, XW128x128x2 | (3 << 27))   # 7 - 3 = 4 stages of phase 1: the shortest that runs


def test_auto_staggers_only_what_its_rule_admits(describe):
    """AUTO's rule (w4a16_plan.hip xw_stagger_auto): the two-slice 128 x 128 launch of 128 tiles with >= 16 stages per slice; every other launch
    is today's."""
    for M, K, N in ((300, 4096, 4096), (512, 2048, 4096), (1024, 4096, 4096), (64, 4096, 4096), (1, 4096, 4096), (4096, 4096, 4096), (160, 4096, 6144)):
        assert "stagger" not in describe(M, K, N, 128)
    for M, K, N in ((512, 4096, 4096), (512, 11008, 4096), (400, 8192, 4096)):
        text = describe(M, K, N, 128)
        assert text.startswith("xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2") and " stagger=1 workspace=" in text, text
