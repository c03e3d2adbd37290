"""The rule by which ``ops.attn_decode*`` choose between the single-launch decode kernels and the
split-KV ones (``ops.DECODE_SPLIT_MIN``), checked without a GPU: the extension is replaced by a
stub that notes which op it was asked for, and the arguments are stand-ins that only carry what
the rule looks at (device, dtype, shape).  CPU and fp32 tensors still reach the oracle."""
import pytest
import torch

from building_llm_from_scratch_amd import ops
from building_llm_from_scratch_amd.ops import reference as ref


class _GpuTensor:
    """What the dispatch reads of a GPU tensor."""

    def __init__(self, *shape, dtype=torch.bfloat16):
        self.shape, self.dtype, self.device = torch.Size(shape), dtype, torch.device("cuda")

    def contiguous(self):
        return self


class _Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return name
        return call


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(ops, "_k", lambda: s)
    monkeypatch.setattr(ops, "load_ext", lambda required=False: True)
    return s


def _call(form, Tmax, L=None, dtype=torch.bfloat16, hd=64):
    B, H, Gk = 2, 4, 2
    kc, vc = _GpuTensor(B, Gk, Tmax, hd, dtype=dtype), _GpuTensor(B, Gk, Tmax, hd, dtype=dtype)
    if form == "plain":
        return ops.attn_decode(_GpuTensor(B, H, hd, dtype=dtype), kc, vc, L)
    qkv = _GpuTensor(B, (H + 2 * Gk) * hd, dtype=dtype)
    if form == "append":
        return ops.attn_decode_append(qkv, kc, vc, _GpuTensor(1, dtype=torch.int32), H, Gk)
    return ops.attn_decode_append_rows(qkv, kc, vc, _GpuTensor(B, dtype=torch.int32), H, Gk)


def test_threshold_is_the_single_launch_kernels_limit():
    assert ops.DECODE_SPLIT_MIN == 8192


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dispatch_on_both_sides_of_the_threshold(stub, dtype):
    M = ops.DECODE_SPLIT_MIN
    # the append forms go by the cache's length
    for Tmax, suffix in ((64, ""), (M, ""), (M + 1, "_split"), (4 * M, "_split")):
        assert _call("append", Tmax, dtype=dtype) == ("attn_decode_append_split" if suffix else "attn_decode_append")
        assert _call("rows", Tmax, dtype=dtype) == ("attn_decode_append_split" if suffix
                                                     else "attn_decode_append_rows")
    # the plain form by the number of keys, whatever the cache could hold
    for Tmax, L, want in ((64, 64, "attn_decode"), (4 * M, 1, "attn_decode"), (4 * M, M, "attn_decode"),
                          (4 * M, M + 1, "attn_decode_split"), (4 * M, 4 * M, "attn_decode_split")):
        assert _call("plain", Tmax, L, dtype=dtype) == want
    assert len(stub.calls) == 13


def test_dispatch_with_the_threshold_at_zero(stub, monkeypatch):
    monkeypatch.setattr(ops, "DECODE_SPLIT_MIN", 0)
    assert _call("append", 64) == "attn_decode_append_split"
    assert _call("rows", 64) == "attn_decode_append_split"
    assert _call("plain", 64, 1) == "attn_decode_split"


def test_cpu_and_fp32_reach_the_oracle(stub, monkeypatch):
    """Lengths on both sides of the threshold (patched low to keep the tensors small)."""
    monkeypatch.setattr(ops, "DECODE_SPLIT_MIN", 8)
    torch.manual_seed(0)
    B, H, Gk, hd = 2, 4, 2, 16
    for Tmax in (8, 24):
        for dt in (torch.float32, torch.bfloat16):
            qkv = torch.randn(B, (H + 2 * Gk) * hd).to(dt)
            kc, vc = torch.randn(B, Gk, Tmax, hd).to(dt), torch.randn(B, Gk, Tmax, hd).to(dt)
            pos = torch.tensor([Tmax - 1, 3], dtype=torch.int32)
            k1, v1 = kc.clone(), vc.clone()
            got = ops.attn_decode_append_rows(qkv, kc, vc, pos, H, Gk)
            want = ref.attn_decode_append_rows(qkv, k1, v1, pos, H, Gk)
            assert torch.equal(got, want) and torch.equal(kc, k1) and torch.equal(vc, v1)
            q = qkv.view(B, H + 2 * Gk, hd)[:, :H]
            assert torch.equal(ops.attn_decode(q, kc, vc, Tmax), ref.attn_decode(q, kc, vc, Tmax))
    # fp32 on the GPU: the per-row form has no kernel and goes to the oracle, not to the extension
    monkeypatch.setattr(ref, "attn_decode_append_rows", lambda *a: "oracle")
    assert _call("rows", 24, dtype=torch.float32) == "oracle"
    assert _call("rows", 24, hd=32) == "oracle"
    assert stub.calls == []
