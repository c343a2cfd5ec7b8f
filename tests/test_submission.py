"""CPU side of the challenge-format output (strajnet_amd/submission.py): quantize_reference -- the reference's three NumPy lines,
inference.py:168-181 -- against an independently written float64 restatement on hand cases, and QuantizedWaypoints on host memory
(layout, raw bytes, zlib round trip, dequantisation error)."""
import zlib

import numpy as np
import torch


def _restated(out):
    """Independent of quantize_reference: float64 sigmoid, np.rint, explicit loops over the waypoint axis."""
    out = np.asarray(out, np.float64)
    B, H, W, C = out.shape
    obs = np.zeros((B, C // 4, H, W), np.uint8)
    occ = np.zeros((B, C // 4, H, W), np.uint8)
    flow = np.zeros((B, C // 4, H, W, 2), np.int8)
    for k in range(C // 4):
        obs[:, k] = np.rint(255.0 / (1.0 + np.exp(-out[..., 4 * k]))).astype(np.uint8)
        occ[:, k] = np.rint(255.0 / (1.0 + np.exp(-out[..., 4 * k + 1]))).astype(np.uint8)
        flow[:, k] = np.minimum(np.maximum(np.rint(out[..., 4 * k + 2:4 * k + 4]), -128), 127).astype(np.int8)
    return obs, occ, flow


def _pack(obs, occ, flow):
    B = obs.shape[0]
    return torch.from_numpy(np.concatenate([obs.reshape(B, -1), occ.reshape(B, -1), flow.view(np.uint8).reshape(B, -1)], 1))


def test_quantize_reference_hand_cases():
    from strajnet_amd import quantize_reference
    out = np.zeros((1, 2, 4, 32), np.float32)
    out[0, 0, 0, 0], out[0, 0, 1, 0], out[0, 0, 2, 0] = 0.0, 40.0, -40.0            # observed, waypoint 0
    out[0, 1, 0, 5], out[0, 1, 1, 5] = 40.0, -40.0                                  # occluded, waypoint 1
    ties = [0.5, 1.5, -0.5, 127.5, -128.5, 300.0, -300.0, 2.5]
    for i, v in enumerate(ties):
        out[0, i // 4, i % 4, 2] = v                                               # flow x, waypoint 0
        out[0, i // 4, i % 4, 31] = -v                                              # flow y, waypoint 7
    obs, occ, flow = quantize_reference(out)
    assert obs.shape == occ.shape == (1, 8, 2, 4) and flow.shape == (1, 8, 2, 4, 2)
    assert obs.dtype == occ.dtype == np.uint8 and flow.dtype == np.int8
    assert obs[0, 0, 0, :3].tolist() == [128, 255, 0]                              # 127.5 is a tie: to even
    assert occ[0, 1, 1, :2].tolist() == [255, 0] and occ[0, 0, 0, 0] == 128
    assert flow[0, 0, :, :, 0].reshape(-1).tolist() == [0, 2, 0, 127, -128, 127, -128, 2]
    assert flow[0, 7, :, :, 1].reshape(-1).tolist() == [0, -2, 0, -128, 127, -128, 127, -2]
    for a, b in zip((obs, occ, flow), _restated(out)):
        assert np.array_equal(a, b)
    rng = np.random.default_rng(3)
    rnd = (rng.standard_normal((2, 8, 16, 32)) * 4).astype(np.float32)
    rnd[..., 2::4] *= 20
    rnd[..., 3::4] *= 20
    got, ref = quantize_reference(rnd), _restated(rnd)
    assert np.array_equal(got[2], ref[2])
    for a, b in zip(got[:2], ref[:2]):                                              # float32 sigmoid against float64: a tie may fall the other way
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1 and (a != b).mean() < 1e-3


def test_flow_slice_byte_order():
    """flow[b, k] is the [1,H,W,2] slice of the reference in C order: x and y of a cell next to each other."""
    from strajnet_amd import quantize_reference
    H, W = 3, 5
    out = np.zeros((1, H, W, 32), np.float32)
    out[0, :, :, 4 * 3 + 2] = np.arange(H * W).reshape(H, W)                       # waypoint 3, x = cell index
    out[0, :, :, 4 * 3 + 3] = -np.arange(H * W).reshape(H, W)                      # y = -cell index
    _, _, flow = quantize_reference(out)
    ref = np.clip(np.round(out[0:1, ..., 14:16]), -128, 127).astype(np.int8).tobytes()
    assert flow[0, 3].tobytes() == ref
    assert list(ref[:6]) == [0, 0, 1, 255, 2, 254]


def test_quantized_waypoints_on_host_memory():
    from strajnet_amd import QuantizedWaypoints, quantize_reference
    B, H, W = 3, 8, 16
    rng = np.random.default_rng(11)
    arr = (rng.standard_normal((B, H, W, 32)) * 3).astype(np.float32)
    arr[..., 2::4] *= 10
    arr[..., 3::4] *= 10
    obs, occ, flow = quantize_reference(arr)
    qw = QuantizedWaypoints(_pack(obs, occ, flow), H, W)
    assert qw.batch == B
    assert np.array_equal(qw.observed.numpy(), obs) and np.array_equal(qw.occluded.numpy(), occ) and np.array_equal(qw.flow.numpy(), flow)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    for b in range(B):
        comp = qw.compressed(b)
        assert len(comp) == 8
        for k in range(8):
            # the reference's own slicing of a batch of one (train.py:105-123 + inference.py:168-181)
            ref = (np.round(sig(arr[b:b + 1, ..., 4 * k:4 * k + 1]) * 255).astype(np.uint8).tobytes(),
                   np.round(sig(arr[b:b + 1, ..., 4 * k + 1:4 * k + 2]) * 255).astype(np.uint8).tobytes(),
                   np.clip(np.round(arr[b:b + 1, ..., 4 * k + 2:4 * k + 4]), -128, 127).astype(np.int8).tobytes())
            raw = qw.waypoint_bytes(b, k)
            assert raw == ref
            assert [len(r) for r in raw] == [H * W, H * W, 2 * H * W]
            for i in range(3):
                assert zlib.decompress(comp[k][i]) == ref[i]
                assert comp[k][i] == zlib.compress(ref[i])
    g = qw.dequantize()
    assert g._packed.shape == (B, H, W, 32) and len(g.vehicles.flow) == 8
    clipped = np.clip(arr, -128, 127)
    # 1/510 holds for the exact sigmoid; the byte comes from a float32 one (3 ulp: a value within 255 * 3 * 6e-8 of a tie may fall the other
    # way, 3.6e-7 more in probability) and q / 255 is a float32 (6e-8)
    SLACK = 5e-7
    for k in range(8):
        assert g.vehicles.observed_occupancy[k].shape == (B, H, W, 1) and g.vehicles.flow[k].shape == (B, H, W, 2)
        assert np.abs(g.vehicles.observed_occupancy[k].numpy()[..., 0] - sig(arr[..., 4 * k].astype(np.float64))).max() <= 1 / 510 + SLACK
        assert np.abs(g.vehicles.occluded_occupancy[k].numpy()[..., 0] - sig(arr[..., 4 * k + 1].astype(np.float64))).max() <= 1 / 510 + SLACK
        assert np.abs(g.vehicles.flow[k].numpy() - clipped[..., 4 * k + 2:4 * k + 4]).max() <= 0.5


def test_quantized_waypoints_rejects_wrong_buffers():
    import pytest
    from strajnet_amd import QuantizedWaypoints, quantize_waypoints
    with pytest.raises(ValueError):
        QuantizedWaypoints(torch.zeros((2, 100), dtype=torch.uint8), 8, 8)
    with pytest.raises(ValueError):
        QuantizedWaypoints(torch.zeros((2, 32 * 64), dtype=torch.int8), 8, 8)
    with pytest.raises(RuntimeError):
        quantize_waypoints(torch.zeros((1, 16, 16, 32)))                            # CPU tensor: no fallback
