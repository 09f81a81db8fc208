"""The guarded-arena harness of the memory-contract tests (tests/_arena.py) can fail: planted stray writes are caught, a clean
use passes, and an input arena's guards read as NaN in both number formats.  Arenas on the CPU; no GPU needed."""
import pytest
import torch

import _arena as A


def test_guard_is_a_multiple_of_256_bytes():
    assert A.GUARD == 64 * 1024 and A.GUARD % 256 == 0


@pytest.mark.parametrize("make", [lambda: A.output_arena((3, 5, 7), torch.float32, "cpu"),
                                  lambda: A.workspace_arena(1001, "cpu"),
                                  lambda: A.input_arena(torch.randn(2, 9), "cpu")])
def test_clean_use_passes(make):
    a = make()
    a.check()
    a.payload.fill_(0x11)                   # every payload byte, first and last included
    a.check()


@pytest.mark.parametrize("nbytes", [420, 1001, 0])
def test_write_just_before_the_payload_is_caught(nbytes):
    a = A.workspace_arena(nbytes, "cpu")
    a.buf[A.GUARD - 1] ^= 0x01
    with pytest.raises(A.GuardError) as e:
        a.check()
    assert "front guard" in str(e.value) and "offsets -1 .. -1" in str(e.value)


@pytest.mark.parametrize("nbytes", [420, 1001, 0])
def test_write_just_after_the_payload_is_caught(nbytes):
    a = A.output_arena((nbytes,), torch.uint8, "cpu")
    a.buf[A.GUARD + nbytes] ^= 0x80
    with pytest.raises(A.GuardError) as e:
        a.check()
    assert "back guard" in str(e.value) and "offsets %d .. %d" % (nbytes, nbytes) in str(e.value)


def test_first_and_last_offending_offsets_are_reported():
    a = A.output_arena((10,), torch.float32, "cpu")
    a.buf[A.GUARD + 40 + 3] = 0
    a.buf[A.GUARD + 40 + 300] = 0
    a.buf[-1] ^= 0xFF
    with pytest.raises(A.GuardError) as e:
        a.check()
    assert "offsets 43 .. %d" % (40 + A.GUARD - 1) in str(e.value)


def test_input_guards_read_as_nan_in_fp32_and_bf16():
    x = torch.randn(4, 6)
    a = A.input_arena(x, "cpu")
    assert torch.equal(a.view(torch.float32, (4, 6)), x)
    for side in ("front", "back"):
        g = a.guard(side)
        assert torch.isnan(g.view(torch.float32)).all()
        assert torch.isnan(g.view(torch.bfloat16).float()).all()
    xb = torch.randn(3, 5).to(torch.bfloat16)
    b = A.input_arena(xb, "cpu")
    assert torch.equal(b.view(torch.bfloat16, (3, 5)).view(torch.int16), xb.view(torch.int16))


def test_output_payload_is_nan_prefilled_and_workspace_is_exact():
    o = A.output_arena((7, 3), torch.float32, "cpu")
    assert o.nbytes == 84 and torch.isnan(o.view(torch.float32)).all() and o.untouched()
    o.view(torch.float32)[0] = 1.0
    assert not o.untouched()
    w = A.workspace_arena(1001, "cpu", fill=A.JUNK_BYTE)
    assert w.nbytes == 1001 and w.buf.numel() == 1001 + 2 * A.GUARD and w.untouched(A.JUNK_BYTE)
    assert w.ptr == w.buf.data_ptr() + A.GUARD
    junk = torch.full((4,), A.JUNK_BYTE, dtype=torch.uint8).view(torch.float32)
    assert torch.isfinite(junk).all()


def test_every_size_query_of_the_header_is_exercised_by_the_contract_table():
    """every *_workspace_bytes / *_records query of include/vcg.h, and every entry point that had no kernel-level test before,
    is named by a row of tests/test_abi_memory_contract_gpu.py"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vcg.h")).read()
    table = open(os.path.join(root, "tests", "test_abi_memory_contract_gpu.py")).read()
    queries = sorted(set(re.findall(r"\b(vcg_\w+(?:_workspace_bytes|_records))\s*\(", header)) - {"vcg_sum_records"})
    assert len([q for q in queries if q.endswith("_workspace_bytes")]) >= 15 and len([q for q in queries if q.endswith("_records")]) >= 5       # the regex still finds them
    first_tested = ["vcg_act_bwd", "vcg_channel_sum", "vcg_sum_records", "vcg_bn_fold", "vcg_bn_fold_batch", "vcg_kernel_transpose",
                    "vcg_sigmoid_gate_fwd", "vcg_sigmoid_gate_bwd", "vcg_atanh_scale", "vcg_dilate2d", "vcg_prelu_bwd_nhwc_bf16",
                    "vcg_prelu_bwd_nhwc_bf16_to_bf16", "vcg_conv9x9_to3_bf16_dgrad_chsum", "vcg_pack_conv3x3_c64_bf16_batch",
                    "vcg_pack_conv_frag_bf16_pair"]
    missing = [q for q in queries + first_tested if not re.search(r"\b%s\b" % q, table)]
    assert not missing, missing
