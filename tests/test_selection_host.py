"""The loss-row selection the statistics-only row list and the filtered transposed CSR are built from
(ops.ce_selection): mask bit(s) AND a label in [0, C) — the predicate of the fused kernel's loss epilogue."""
import torch

from rgb_experiment_amd import ops


def test_selection_is_mask_and_label_in_range():
    y = torch.tensor([0, 3, -1, 4, 2, 7, 1])
    mask = torch.tensor([1, 1, 1, 1, 0, 1, 1], dtype=torch.bool)
    assert ops.ce_selection(y, mask, 4).tolist() == [True, True, False, False, False, False, True]
    assert ops.ce_selection(y, None, 4).tolist() == [True, True, False, False, True, False, True]


def test_grouped_mask_selects_the_union():
    y = torch.tensor([0, 1, 2, 3, 9])
    grouped = torch.tensor([0, 1, 2, 3, 3], dtype=torch.uint8)  # bit 0 / bit 1 = the two masks (ops.group_masks)
    assert ops.ce_selection(y, grouped, 4).tolist() == [False, True, True, True, False]
