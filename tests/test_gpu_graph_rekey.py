"""GPU tests of the captured launch sequences (RcGraphCache, csrc/rcflow_api.hip) when their key changes: a call with other
buffers drops the captured graph of its ring parity, runs eagerly, and the next call with the same buffers captures again.
Same bits as the eager launches throughout."""
import numpy as np
import pytest
import torch

from ripcurrents_amd import synth

pytestmark = pytest.mark.gpu
W, H = 96, 64
PRM = dict(pyr_scale=0.5, levels=2, winsize=3, poly_n=15, poly_sigma=1.2, flags=0)


def test_push_batch_captures_again_after_other_buffers(ctx):
    """Two lockstep streams.  On one pair of tensors: prime, eager and eager (one per ring parity), capture and capture, replay
    and replay.  Then other tensors of the same shape: both parities find another key (eager, the old graphs dropped),
    capture again, replay."""
    S, first, second = 2, 7, 6
    clips = np.stack([synth.surf_clip(W, H, first + second, seed=300 + s) for s in range(S)])      # [S,T,h,w]
    d = torch.as_tensor(clips).cuda()
    bufs = [(torch.empty((S, H, W), dtype=torch.uint8, device="cuda"), torch.empty((S, H, W, 2), dtype=torch.float32, device="cuda"))
            for _ in range(2)]

    def run(use_graph):
        ctx.batch_reset()
        got = []
        for t in range(first + second):
            frames, flows = bufs[t >= first]
            frames.copy_(d[:, t])
            r = ctx.push_batch(frames, flows, use_graph=use_graph, iterations=2, **PRM)
            assert (r is None) == (t == 0)
            if r is not None:
                ctx.sync()
                got.append(r.cpu().numpy().copy())
        ctx.batch_reset()
        return got

    ref, got = run(False), run(True)
    assert len(ref) == len(got) == first + second - 1
    for t, (a, b) in enumerate(zip(ref, got)):
        assert np.abs(a).max() > 0 and np.array_equal(a, b), "flow %d" % t


def test_frame_loop_step_captures_again_after_another_edges_buffer(ctx):
    """Six frames through rcflow_frame_loop_step with use_graph (prime, eager x 2, capture x 2, replay), then four more that
    write the edges to another tensor: another key on both parities, eager, then captured again.  Flow, mask and both edge
    images after every frame equal the run without graphs."""
    first, second = 6, 4
    clip = synth.surf_clip(W, H, first + second, seed=77)

    def run(use_graph):
        ctx.stream_reset()
        ctx.analysis_reset(W, H)
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        edges = [torch.zeros((H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
        snaps = []
        for t in range(first + second):
            ctx.frame_buffer(W, H)[:] = clip[t]
            f = ctx.frame_loop_step(W, H, outmask=mask, edges=edges[t >= first], use_graph=use_graph, iterations_flow=2, **PRM)
            assert (f is None) == (t == 0)
            if f is not None:
                ctx.sync()
                snaps.append([x.cpu().numpy().copy() for x in (f, mask, edges[0], edges[1])])
        ctx.stream_reset()
        return snaps

    ref, got = run(False), run(True)
    assert len(ref) == len(got) == first + second - 1
    for t, (a, b) in enumerate(zip(ref, got)):
        for name, x, y in zip(("flow", "outmask", "edges", "edges after the switch"), a, b):
            assert np.array_equal(x, y), "frame %d: %s" % (t + 1, name)
    assert np.abs(ref[-1][0]).max() > 0
