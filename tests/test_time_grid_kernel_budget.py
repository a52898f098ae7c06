"""Register / spill / scratch / LDS ceilings of the per-instance kernels (sa_k_forward_t, sa_k_backward_t,
sa_k_sens_t: the launch form of every kernel body that reads each instance's own start time and output grid).
profiles/code_object_budget.json holds the shared-time kernels of the same code objects; these ceilings are recorded
here, with the same slack and the same occupancy-class rule (tools/code_object_budget.py), so that a regression of the
per-instance path fails a CPU test too."""
import pytest

from tools import code_object_budget as cob

#: label -> kernel -> (vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size,
#: vgpr_count, agpr_count), as built when the per-instance kernels were introduced
RECORDED = {
    "lv": {"sa_k_forward_t": (0, 0, 0, 0, 228, 0), "sa_k_backward_t": (0, 12, 0, 0, 366, 110)},
    "robertson": {"sa_k_forward_t": (0, 64, 0, 4608, 233, 0), "sa_k_backward_t": (30, 14, 0, 17920, 414, 158)},
    "seir": {"sa_k_forward_t": (24, 114, 0, 40720, 468, 212), "sa_k_backward_t": (93, 152, 160, 40720, 512, 256)},
    "network24": {"sa_k_forward_t": (14, 278, 0, 24216, 297, 41), "sa_k_backward_t": (22, 274, 0, 24216, 400, 144)},
    "network100": {"sa_k_forward_t": (86, 126, 256, 103120, 397, 141),
                   "sa_k_backward_t": (106, 161, 288, 103120, 479, 223)},
    "lv/sens": {"sa_k_forward_t": (0, 0, 0, 0, 228, 0), "sa_k_sens_t": (138, 6, 0, 0, 483, 227)},
    "robertson/sens": {"sa_k_forward_t": (0, 0, 0, 4608, 272, 16), "sa_k_sens_t": (1088, 40, 1168, 4608, 512, 256)},
    "seir/sens": {"sa_k_forward_t": (118, 126, 192, 38928, 512, 256), "sa_k_sens_t": (623, 160, 1120, 38920, 512, 256)},
}


def test_recorded_labels_are_the_budgeted_builds():
    assert set(RECORDED) == set(cob.BUILDS)


@pytest.mark.parametrize("label", sorted(RECORDED))
def test_per_instance_kernels_stay_within_their_ceilings(label):
    """(cross-compiles for gfx950 on the CPU box; cached after the first build)"""
    from sunode_amd import _native
    problem, kw = cob.BUILDS[label]
    notes = _native.code_object_notes(_native.build_code_object(cob.source_of(problem), **kw))
    for kernel, values in RECORDED[label].items():
        assert kernel in notes, (label, kernel)
        rec = dict(zip(cob.FIELDS, values))
        got = notes[kernel]
        for f in cob.HARD_FIELDS:
            assert got[f] <= rec[f] + cob.SLACK[f], (label, kernel, f, got[f], rec[f])
        assert cob.register_class(got) >= cob.register_class(rec), (label, kernel, got)
    if label.startswith("lv"):          # Lotka-Volterra: no spill slots, no scratch, like its shared-time kernels
        for kernel in ("sa_k_forward_t", "sa_k_backward_t"):
            if kernel in notes:
                assert notes[kernel]["vgpr_spill_count"] == 0 and notes[kernel]["private_segment_fixed_size"] == 0
