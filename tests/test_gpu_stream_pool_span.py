"""The one commit body and the one vote body of csrc/stream_pool.hip under both id-span policies, on the smallest pool where a window
boundary falls inside the burst: capacity 4, vote window 3, max_events 8, 2 slots, 4 frames each.  The raw vote records - and the host
model's words for the reference ids - must be equal after
  (a) push_frames with K = 4            pool_commit<UniformSpan>, K = 4
  (b) push_ragged with counts [4, 4]    pool_commit<RaggedSpan>
  (c) four push calls                   pool_commit<UniformSpan>, K = 1
on the saturated-gate automaton, whose ids are the reference's on every route (a two-slot `push` takes `step`'s fused LayerNorm, other
bits on real weights), and, for the Transformer pool, after
  (d) push_bursts with counts [4, 4]    pool_vote<RaggedSpan>
against a record fed the ids push_bursts returned through `vote`, one frame per call (pool_vote<UniformSpan>, K = 1).
(a) = (c) and (b) = (c) are also held pairwise, on real weights and larger pools, by tests/test_gpu_stream_pool_frames.py::
test_push_frames_equals_k_pushes_on_real_weights and tests/test_gpu_stream_pool_ragged.py::test_push_ragged_equals_per_slot_pushes_on_real_weights."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd.aggregate import OnlineRecord                          # noqa: E402
from prego_amd.engine import MiniRoadEngine                           # noqa: E402
from prego_amd.stream_pool import StreamPool, pack_bursts             # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  its references are computed once and shared
from tests.helpers import stream_refusal_cases as R                   # noqa: E402

DEV = "cuda:0"
CAP, WINDOW, EVENTS, K = 4, 3, 8, 4
SLOTS = (2, 0)


def _raw_record(pool, slot):
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert getattr(pool.lib, pool._C["record"])(pool.p, slot, C.byref(ptr), C.byref(nb)) == 0
    off = ptr.value - pool._block.data_ptr()
    return pool._block[off:off + nb.value].view(torch.int32).cpu().tolist()


def _opened(pool):
    for _ in range(3):
        pool.open()
    return pool


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_frames_ragged_and_single_pushes_leave_the_same_records(dtype):
    case, sd, n, T, x, res = TW._ref("L4-C12")
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, case.n_classes, DEV, dtype)
    e.set_weights(sd)
    frames, ragged, single = (_opened(StreamPool(e, capacity=CAP, window=WINDOW, max_events=EVENTS)) for _ in range(3))
    streams = (5, 11)
    burst = x[list(streams), :K].contiguous()                                    # [2, K, d_rgb]
    a = frames.push_frames(SLOTS, burst, None, softmax=False, want_ant=False)
    b = ragged.push_ragged(SLOTS, [K, K], pack_bursts([burst[0], burst[1]])[0], None, softmax=False, want_ant=False)
    c = [single.push(SLOTS, burst[:, t].contiguous(), None, softmax=False, want_ant=False) for t in range(K)]
    ids = res.argmax.view(n, T)[list(streams), :K].to(torch.int32)
    assert torch.equal(a[1], ids) and torch.equal(b[1].view(2, K), ids) and torch.equal(torch.stack([t[1] for t in c], dim=1), ids)
    for i, slot in enumerate(SLOTS):
        model = OnlineRecord(WINDOW, case.n_classes, EVENTS)
        model.push_frames(ids[i].tolist())
        want = model.to_words()
        assert want[0] == K and want[2] == 1 and sum(want[4:4 + case.n_classes]) == K - WINDOW      # one window voted inside the burst, one id pending
        got = [_raw_record(p, slot) for p in (frames, ragged, single)]
        assert got[0] == want and got[1] == want and got[2] == want, f"slot {slot}"
        assert torch.equal(frames.state(slot), ragged.state(slot)) and torch.equal(frames.state(slot), single.state(slot))
    assert all(_raw_record(p, 1) == [0] * len(want) for p in (frames, ragged, single))              # the open slot nobody named
    e.check()


def test_transformer_bursts_vote_as_the_same_ids_through_vote():
    vit = R.Ctx(DEV).vit("flow")
    pool = _opened(vit.stream_pool(capacity=CAP, vote_window=WINDOW, max_events=EVENTS))
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    rgb, flow = (torch.randn((2 * K, d), device=DEV, generator=g).clamp_(min=0) for d in (vit.d_rgb, vit.d_flow))
    ids = pool.push_bursts(SLOTS, [K, K], rgb, flow)[1].view(2, K)
    # a record of the same layout (classes, max_events) on a handle without weights: `vote` serves every engine
    voted = _opened(StreamPool(MiniRoadEngine(2048, 0, 2048, 1024, vit.out_dim, DEV, "bf16"), capacity=CAP, window=WINDOW, max_events=EVENTS))
    for t in range(K):
        voted.vote(SLOTS, ids[:, t].contiguous())
    for i, slot in enumerate(SLOTS):
        model = OnlineRecord(WINDOW, vit.out_dim, EVENTS)
        model.push_frames(ids[i].tolist())
        want = model.to_words()
        assert want[0] == K and want[2] == 1
        assert _raw_record(pool, slot) == want and _raw_record(voted, slot) == want, f"slot {slot}"
