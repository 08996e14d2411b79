"""fp32 mode: the reference WITHOUT --amp (ddp/trainer.py:160-165, single/trainer.py:144-145) trains
plain fp32; north_star holds per-layer activations and gradients to 1e-5 relative there. The native
executor runs that path (outside `autocast`) on f32-input MFMA convolutions (conv_f32.hip) and fp32
BN / head kernels; every check here is against the fp32 oracle (float64 arithmetic on the
executor's own fp32 inputs)."""
import numpy as np
import pytest
import torch

from oracle import resnet as R
from tests.conftest import rel_err
from tests.test_gpu_resnet import ODD_SIZES, _hw, _np, _setup, _split_state, _teacher_forced

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", [2, 8])
def test_fp32_per_layer_teacher_forced(dtc, cuda, batch):
    """Every layer's forward output and backward intermediate, and every parameter gradient, of
    the fp32 executor within 1e-5 of the oracle on that layer's inputs (129 checks)."""
    errs = _teacher_forced(dtc, cuda, batch, precision="fp32")
    assert len(errs) > 90


def test_fp32_per_layer_teacher_forced_b64_224(dtc, cuda):
    """fp32 at a split-K-heavy shape (batch 64: wgrad splits, many tiles) on layers 3-4 + head, and at
    224x224 batch 1 on every layer (large images: multi-tile rows, int64 offsets)."""
    _teacher_forced(dtc, cuda, 64, stages=(0, 3, 4), imgs=np.arange(0, 64, 7), seed=31, precision="fp32")
    _teacher_forced(dtc, cuda, 1, hw=224, seed=32, precision="fp32")


@pytest.mark.parametrize("num_classes", [10, 1000])
def test_fp32_per_layer_teacher_forced_class_counts(dtc, cuda, num_classes):
    """The fp32 head templates off 100 classes (reachable only through the network): stem, layer4 and the head at
    10 and 1000 classes, the Linear's gradients element-wise."""
    errs = _teacher_forced(dtc, cuda, 3, stages=(0, 4), seed=41, precision="fp32", num_classes=num_classes)
    assert len(errs) >= 30


def test_fp32_per_layer_teacher_forced_non_square(dtc, cuda):
    """24x40 input (maps 24x40 ... 3x5, a 15-pixel pool), every layer, fp32."""
    errs = _teacher_forced(dtc, cuda, 3, hw=(24, 40), seed=43, precision="fp32")
    assert len(errs) > 90


@pytest.mark.parametrize("batch,hw,seed", ODD_SIZES, ids=["18x21", "28x28", "15x17"])
def test_fp32_per_layer_teacher_forced_odd_extents(dtc, cuda, batch, hw, seed):
    """Sizes whose stride-2 blocks see odd maps (tests/test_gpu_resnet.py::ODD_SIZES), every layer, fp32."""
    errs = _teacher_forced(dtc, cuda, batch, hw=hw, seed=seed, precision="fp32")
    assert len(errs) > 90


def test_fp32_end_to_end_matches_oracle(dtc, cuda):
    """Free-running fp32 forward + backward vs the fp32 oracle (no rounding points anywhere): unlike
    bf16, fp32 stays close end to end -- logits and loss to 1e-5, every activation to 1e-4, every
    parameter gradient to 1e-3 (measured drift is fp32 summation order only), running statistics
    to 1e-5."""
    _fp32_end_to_end(dtc, cuda, 8, 32)


def test_fp32_end_to_end_matches_oracle_odd_extents(dtc, cuda):
    """The same free-running step, with the same bounds, at 18x21 batch 3: every stride-2 block sees an odd map
    (even/odd, odd/odd, odd/even)."""
    _fp32_end_to_end(dtc, cuda, 3, (18, 21))


def _fp32_end_to_end(dtc, cuda, batch, hw):
    model, sd, x, y = _setup(dtc, cuda, batch, seed=4, hw=hw)
    model.precision = "fp32"
    crit = dtc.CrossEntropyLoss()
    logits = model(torch.from_numpy(x).to(cuda))
    loss = crit(logits, torch.from_numpy(y).to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    params, bufs = _split_state(sd)
    ref = R.forward_backward(params, bufs, x, y, bf16_mode=False, train=True, want_acts=True)
    assert rel_err(_np(logits), ref["logits"]) < 1e-5
    assert abs(float(loss) - ref["loss"]) < 1e-5 * max(1.0, abs(ref["loss"]))
    acts = model.executor(batch, *_hw(hw), "fp32").activations()
    for k, v in ref["acts"].items():
        e = rel_err(_np(acts[k]).reshape(v.shape), v)
        assert e < 1e-4, (k, e)
    worst = 0.0
    for k, p in model.named_parameters():
        e = rel_err(_np(p.grad), ref["grads"][k])
        worst = max(worst, e)
        # fp32 summation-order noise amplified through 20 layers of backward: measured 1.1e-3 on the
        # stem weight gradient (the deepest), <= 1e-4 from layer2 on
        assert e < 5e-3, (k, e)
    print(f"fp32 end-to-end worst parameter-gradient drift vs the fp64 oracle: {worst:.2e}")
    sd2 = model.state_dict()
    for k, v in ref["buffers"].items():
        e = rel_err(sd2[k].cpu().numpy(), v)
        assert e < 1e-5, (k, e)


def test_fp32_data_parallel_step_matches_oracle(dtc, cuda):
    """DataParallel (reference src/dp/trainer.py:27, torch nn.DataParallel semantics) with two replicas on
    cuda:0 (device_ids=[0, 0]) against the fp32 oracle: each replica runs train-mode BN over its own
    half of the batch (the oracle's forward on that half), so the gathered logits are the two halves'
    oracle logits (1e-5) and the mean loss over the whole batch is the mean of the halves' losses; the
    running statistics are replica 0's update (1e-5; the module is replica 0, replica 1's buffers are
    discarded, as torch's replicate does). A DP that normalised over the whole 16-image batch instead of
    per replica fails the logits check.
    Gradient: the DP backward scatters dlogits, runs each replica's backward on its slice and reduce-adds
    the replicas' flat gradients. With the same dlogits (the mean cross-entropy's, fed explicitly) the
    module's gradient must equal, bit for bit, the sum of the same executor's single-replica backwards on
    each half (the step is deterministic; a two-term fp32 sum has one order); the single-replica backward
    itself is pinned to the oracle per layer at 1e-5 by test_fp32_per_layer_teacher_forced."""
    B = 8
    model, sd, x, y = _setup(dtc, cuda, 2 * B, seed=6)
    model.precision = "fp32"
    crit = dtc.CrossEntropyLoss()
    params, bufs = _split_state(sd)
    halves = [R.forward_backward(params, bufs, x[h * B:(h + 1) * B], y[h * B:(h + 1) * B], bf16_mode=False,
                                 train=True) for h in range(2)]
    dp = dtc.DataParallel(model, device_ids=[0, 0])
    dp.zero_grad()
    logits = dp(torch.from_numpy(x).to(cuda))
    loss = crit(logits, torch.from_numpy(y).to(cuda))
    torch.cuda.synchronize()
    assert rel_err(_np(logits), np.concatenate([r["logits"] for r in halves])) < 1e-5
    ref_loss = 0.5 * (halves[0]["loss"] + halves[1]["loss"])
    assert abs(float(loss) - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
    # dlogits of the mean cross-entropy over the 16 rows (trainer.py:155), fed to both paths
    p = torch.softmax(logits.detach().double(), 1)
    p[torch.arange(2 * B), torch.from_numpy(y).to(cuda)] -= 1.0
    dl = (p / (2 * B)).float().contiguous()
    logits.backward(dl)
    torch.cuda.synchronize()
    single = []  # the executor's own gradients on each half, from the same dlogits slice
    for h in range(2):
        torch.manual_seed(42)
        m1 = dtc.ResNet18().to(cuda)
        m1.precision = "fp32"
        m1(torch.from_numpy(x[h * B:(h + 1) * B]).to(cuda)).backward(dl[h * B:(h + 1) * B].clone())
        torch.cuda.synchronize()
        single.append({k: _np(p_.grad) for k, p_ in m1.named_parameters()})
        del m1
    worst = (0.0, "")
    for k, p_ in model.named_parameters():
        g = _np(p_.grad)
        np.testing.assert_array_equal(g, single[0][k] + single[1][k], err_msg=k)
        ref = 0.5 * (halves[0]["grads"][k] + halves[1]["grads"][k])
        worst = max(worst, (rel_err(g, ref), k))
    print(f"DP [0,0] fp32: gradient == sum of the replicas' single-run gradients (bit for bit); "
          f"vs the fp64 oracle worst parameter {worst[0]:.2e} ({worst[1]})")
    sd2 = model.state_dict()
    for k, v in halves[0]["buffers"].items():
        e = rel_err(sd2[k].cpu().numpy(), v)
        assert e < 1e-5, (k, e)
    assert int(sd2["bn1.num_batches_tracked"]) == 1


def test_autocast_selects_executor_precision(dtc, cuda):
    """torch semantics at the boundary: inside dtc.autocast() the bf16 executor, outside it fp32
    (what the reference's trainer does with and without --amp); `precision` forces one."""
    torch.manual_seed(42)
    model = dtc.ResNet18().to(cuda)
    x = torch.randn(4, 3, 32, 32, device=cuda)
    with torch.no_grad():
        lo32 = model(x)
        with dtc.autocast():
            lo16 = model(x)
            with dtc.autocast(enabled=False):
                lo32b = model(x)
    keys = sorted(model._executors)
    assert [k[3] for k in keys] == ["bf16", "fp32"]
    assert torch.equal(lo32, lo32b)
    assert 1e-6 < rel_err(_np(lo16), _np(lo32)) < 3e-2  # same network, bf16 rounding only
    model.precision = "bf16"
    with torch.no_grad():
        assert torch.equal(model(x), lo16)


@pytest.mark.parametrize("graphs", [1, 0])
def test_fp32_sgd_steps_graph_and_eager(dtc, cuda, graphs):
    """Three fp32 training steps (forward, backward, fused SGD) with graph replay and eagerly: the
    same numbers (graph replay changes nothing but launch overhead), finite decreasing-ish loss."""
    _graphs_prev = dtc._native.lib.dtc_get_option(b"graphs")
    dtc._native.lib.dtc_set_option(b"graphs", graphs)
    try:
        torch.manual_seed(42)
        model = dtc.ResNet18().to(cuda)
        crit = dtc.CrossEntropyLoss()
        opt = dtc.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
        g = torch.Generator().manual_seed(8)
        x = torch.randn(16, 3, 32, 32, generator=g).to(cuda)
        y = torch.randint(0, 100, (16,), generator=g).to(cuda)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = crit(model(x), y)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
        test_fp32_sgd_steps_graph_and_eager.results[graphs] = (losses, _np(model.flat.params))
    finally:
        dtc._native.lib.dtc_set_option(b"graphs", _graphs_prev)
    res = test_fp32_sgd_steps_graph_and_eager.results
    if len(res) == 2:
        np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)
        assert rel_err(res[0][1], res[1][1]) < 1e-7


test_fp32_sgd_steps_graph_and_eager.results = {}


def test_trainer_without_amp_trains_fp32(dtc, cuda, tmp_path):
    """`train.py single` without --amp (single/trainer.py:144-145): the loop runs the fp32 executor
    (no GradScaler), like the reference."""
    t = dtc.trainer.main(["--epoch", "1", "--batch-size", "32", "--max-steps", "3", "--workers", "0",
                          "--synthetic-train", "320", "--synthetic-test", "64", "--eval-step", "1",
                          "--ckpt-path", str(tmp_path)], "single")
    precs = {k[3] for k in t.model._executors}
    assert precs == {"fp32"}, precs
