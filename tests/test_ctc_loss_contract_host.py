"""Host side of nn.CTCLoss's full contract (blank, reduction, zero_infinity, target layouts, length types, unbatched input): what runs
without a GPU -- construction, argument validation and ops.ctc_prepare, the pure normalisation in front of the kernels."""
import pytest
import torch

from ctc_pytorch_amd import nn, ops


@pytest.mark.parametrize("kw", [{}, {"reduction": "mean"}, {"blank": 5, "zero_infinity": True}, {"reduction": "none"},
                                {"reduction": "sum"}])
def test_ctc_loss_constructs_with_torch_arguments(kw):
    m = nn.CTCLoss(**kw)
    ref = torch.nn.CTCLoss(**kw)
    assert (m.blank, m.reduction, m.zero_infinity) == (ref.blank, ref.reduction, ref.zero_infinity)


def test_ctc_loss_default_is_torch_default():
    m = nn.CTCLoss()
    assert (m.blank, m.reduction, m.zero_infinity) == (0, "mean", False)


def test_ctc_loss_rejects_unknown_reduction():
    with pytest.raises(ValueError):
        nn.CTCLoss(reduction="foo")
    with pytest.raises(ValueError):
        ops.ctc_loss(torch.zeros(4, 2, 3), torch.ones(2, 1, dtype=torch.int64), [4, 4], [1, 1], reduction="elementwise_mean")


def test_ctc_loss_has_no_cpu_fallback():
    lp = torch.log_softmax(torch.randn(6, 2, 5), -1)
    for kw in ({}, {"reduction": "none"}, {"blank": 4, "zero_infinity": True}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            nn.CTCLoss(**kw)(lp, torch.tensor([[1, 2], [3, 0]]), torch.tensor([6, 5]), torch.tensor([2, 1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nn.CTCLoss()(lp[:, 0], torch.tensor([1, 2]), 6, 2)


def test_prepare_padded_targets_keeps_layout_and_lmax():
    lp = torch.zeros(7, 3, 5)
    tg = torch.tensor([[1, 2, 0, 0], [3, 3, 3, 0], [4, 0, 0, 0]])
    a = ops.ctc_prepare(lp, tg, torch.tensor([7, 6, 5]), torch.tensor([2, 3, 1]))
    assert not a.flat and a.batched and a.Lmax == 4 and a.targets is tg and a.lp is lp
    assert a.in_len.dtype == torch.int64 and a.tgt_len.tolist() == [2, 3, 1]


@pytest.mark.parametrize("kind", ["list", "tuple", "tensor", "int32"])
def test_prepare_accepts_lengths_as_list_tuple_tensor(kind):
    lp = torch.zeros(7, 2, 5)
    il, tl = [7, 4], [2, 1]
    conv = {"list": list, "tuple": tuple, "tensor": torch.tensor, "int32": lambda v: torch.tensor(v, dtype=torch.int32)}[kind]
    a = ops.ctc_prepare(lp, torch.tensor([[1, 2], [3, 0]]), conv(il), conv(tl))
    assert a.in_len.dtype == torch.int64 and a.tgt_len.dtype == torch.int64
    assert a.in_len.tolist() == il and a.tgt_len.tolist() == tl


def test_prepare_concatenated_targets_take_lmax_from_the_lengths():
    lp = torch.zeros(9, 3, 6)
    flat = torch.tensor([1, 2, 3, 4, 5, 5, 1])          # lengths 3 + 0 + 4
    a = ops.ctc_prepare(lp, flat, [9, 9, 8], torch.tensor([3, 0, 4]))
    assert a.flat and a.Lmax == 4 and a.targets is flat
    # more targets than the lengths use: accepted, the tail is never read
    assert ops.ctc_prepare(lp, torch.cat([flat, flat]), [9, 9, 8], [3, 0, 4]).Lmax == 4
    # all-empty labels
    assert ops.ctc_prepare(lp, torch.zeros(0, dtype=torch.int64), [9, 9, 8], [0, 0, 0]).Lmax == 0


def test_prepare_rejects_more_target_lengths_than_targets():
    lp = torch.zeros(9, 2, 6)
    with pytest.raises(ValueError, match="sum\\(target_lengths\\)"):
        ops.ctc_prepare(lp, torch.tensor([1, 2, 3]), [9, 9], [2, 2])
    with pytest.raises(ValueError):
        ops.ctc_prepare(lp, torch.tensor([1, 2, 3]), [9, 9], [-1, 2])


def test_prepare_unbatched_input():
    lp = torch.zeros(8, 5)
    for il, tl in ((8, 3), (torch.tensor(8), torch.tensor(3)), (torch.tensor([8]), torch.tensor([3])), ([8], (3,))):
        a = ops.ctc_prepare(lp, torch.tensor([1, 2, 2]), il, tl)
        assert not a.batched and a.flat and tuple(a.lp.shape) == (8, 1, 5) and a.Lmax == 3
        assert a.in_len.tolist() == [8] and a.tgt_len.tolist() == [3]
    with pytest.raises(ValueError):
        ops.ctc_prepare(lp, torch.tensor([1, 2, 2]), [8, 8], [3, 3])


def test_prepare_checks_host_lengths_and_shapes():
    lp = torch.zeros(7, 2, 5)
    tg = torch.tensor([[1, 2], [3, 0]])
    for il, tl in (([8, 4], [2, 1]), ([7, -1], [2, 1]), ([7, 4], [3, 1]), ([7, 4], [2, -1])):
        with pytest.raises(ValueError):
            ops.ctc_prepare(lp, tg, il, tl)
    with pytest.raises(ValueError, match="batch size mismatch"):
        ops.ctc_prepare(lp, tg, [7, 4, 4], [2, 1, 1])
    with pytest.raises(ValueError, match="batch size mismatch"):
        ops.ctc_prepare(lp, tg[:1], [7, 4], [2, 1])
    with pytest.raises(ValueError):
        ops.ctc_prepare(torch.zeros(7), tg, [7], [2])
    with pytest.raises(ValueError):
        ops.ctc_prepare(lp, tg.view(2, 2, 1), [7, 4], [2, 1])


def test_new_entry_points_reject_bad_blank_and_reduction_without_a_gpu():
    """blank outside [0, V), an unknown reduction and an unknown gradient-scale stride are refused by the C ABI before it touches the
    device (all pointers non-null, the dims valid)."""
    import __graft_entry__ as ge
    from ctc_pytorch_amd import _lib
    import os
    if not os.path.exists(_lib.SO_PATH):
        ge.build()
    L = _lib.lib()
    buf = torch.zeros(1 << 12)
    p, q = buf.data_ptr(), buf.data_ptr() + 8192
    T, B, V, Lmax = 4, 2, 5, 2
    for blank in (-1, V, V + 3):
        assert L.ctcn_ctc_fwd_ex(p, p, p, p, p, q, p, T, B, V, Lmax, blank, None) == -1
        assert b"blank" in L.ctcn_last_error()
        assert L.ctcn_ctc_grad_ex(p, p, p, p, p, p, p, p, 0, 2, 0, blank, p, T, B, V, Lmax, None) == -1
    for red in (-1, 3, 7):
        assert L.ctcn_ctc_grad_ex(p, p, p, p, p, p, p, p, 0, red, 0, 0, p, T, B, V, Lmax, None) == -1
        assert b"reduction" in L.ctcn_last_error()
        assert L.ctcn_ctc_reduce(p, p, p, B, red, 0, None) == -1
    assert L.ctcn_ctc_grad_ex(p, p, p, p, p, p, p, p, 2, 0, 0, 0, p, T, B, V, Lmax, None) == -1
    assert L.ctcn_ctc_fwd_ex(p, p, p, p, p, p, p, T, B, V, Lmax, 0, None) == -1          # alpha and beta the same buffer
    assert L.ctcn_ctc_reduce(p, None, p, B, 1, 0, None) == -1                            # 'mean' needs the target lengths
    assert L.ctcn_ctc_pack_targets(p, -1, p, p, B, Lmax, None) == -1
    assert L.ctcn_ctc_pack_targets(p, 4, p, p, B, 0, None) == -1
