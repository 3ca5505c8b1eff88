"""Reference weight formats round-trip into the engine's model (CPU only)."""
import numpy as np
import torch

from channelestimationtransformer_amd.checkpoint import export_json, import_json, load_checkpoint, save_checkpoint
from channelestimationtransformer_amd.informer import InformerStack
from golden_util import load_case


def _model():
    return InformerStack(16, 16, 16, 90, 10, 5, 5, 128, 8, [4], 3, 64, 0.05, "prob", "fixed", "gelu", False, True,
                         torch.device("cpu"))


def test_pt_checkpoint_dict_roundtrip(tmp_path):
    case = load_case("informer_prob_b1")
    p = str(tmp_path / "tmodel_49.pt")
    save_checkpoint(p, case.state, epoch=49, global_step=1234)
    raw = torch.load(p, weights_only=True)
    assert set(raw) == {"epoch", "model_state_dict", "optimizer_state_dict", "global_step"}
    state = load_checkpoint(p)
    m = _model()
    # the callers load with strict=False (QuantizationAwareTraining.py:200)
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in case.state.items():
        np.testing.assert_array_equal(m.state_dict()[k].numpy(), v)


def test_bare_state_dict_file(tmp_path):
    case = load_case("transformer_c3")
    p = str(tmp_path / "sd.pt")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in case.state.items()}, p)
    state = load_checkpoint(p)
    assert set(state) == set(case.state)


def test_json_export_roundtrip(tmp_path):
    case = load_case("informer_prob_b1")
    d = str(tmp_path / "weight_export")
    export_json(case.state, d)
    back = import_json(d)
    assert set(back) == set(case.state)
    for k, v in case.state.items():
        np.testing.assert_array_equal(back[k], v)


def test_trained_mimo_checkpoint_drops_into_the_engine():
    """The only trained weights in the reference (MimoSimulation/models/checkpoint/checkpoint.pth,
    loaded by MimoSimulation/Predict.py:91-93 for InformerStack(16,16,16, 25,10,5, 5, d_model 64, 8,
    e_layers [4,3], 3, 64, attn "full")): read with torch.load(weights_only=True), loaded with the
    callers' strict=False, and planned by the layer-wise engine (d_model 64 is outside the fused
    kernels).  Host only.  The 4.1 MB file is committed as fixture parts of the same format
    (tests/golden/mimo_checkpoint.part*.pth, golden_util.load_mimo_checkpoint)."""
    from channelestimationtransformer_amd.engine import Engine
    from golden_util import load_mimo_checkpoint

    sd = load_mimo_checkpoint()
    assert len(sd) == 239 and sum(v.numel() * v.element_size() for v in sd.values()) == 4052840
    m = InformerStack(16, 16, 16, 25, 10, 5, 5, 64, 8, [4, 3], 3, 64, 0.05, "full", "fixed", "gelu", True, True,
                      torch.device("cpu"))
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    assert all(".temporal_embedding." in k for k in res.missing_keys)   # unused tables (embed.py:132-135)
    eng = Engine.informer(m.config())
    eng.load_state_dict({k: v.numpy() for k, v in m.state_dict().items()})
    assert eng.precision() == "fp32-layerwise"
    assert [L for _, L in eng.attns_layout()] == [25, 13, 7, 4, 12, 6, 3]


def test_weight_staleness_check_is_cheap_and_complete():
    """The per-forward check that decides whether the engine's packed weights are stale (informer.py
    _version) sees in-place edits, load_state_dict and parameter re-assignment, ignores unrelated module
    construction, and does not walk the state_dict on every call (the TimingAnalysis batch-1 harness
    times the model call with its Python dispatch)."""
    import time

    m = _model().eval()
    v0 = m._version()
    t = time.perf_counter()
    for _ in range(200):
        assert m._version() == v0
    per_call = (time.perf_counter() - t) / 200
    t = time.perf_counter()
    for _ in range(20):
        m.state_dict()
    walk = (time.perf_counter() - t) / 20
    assert per_call < walk / 5, (per_call, walk)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        m.projection.weight.add_(1.0)
    v1 = m._version()
    assert v1 != v0
    m.load_state_dict(sd)
    v2 = m._version()
    assert v2 != v1
    m.projection.bias = torch.nn.Parameter(m.projection.bias.detach().clone(), requires_grad=False)
    v3 = m._version()
    assert v3 != v2
    with torch.no_grad():
        m.projection.bias.add_(1.0)       # an in-place edit of a re-assigned (non-flat) parameter
    v4 = m._version()
    assert v4 != v3
    with torch.no_grad():
        m.decoder.norm.weight.mul_(2.0)   # and of one still backed by the flat tensor
    v5 = m._version()
    assert v5 != v4
    torch.nn.Linear(3, 3)   # another module's registrations do not invalidate this one
    assert m._version() == v5


def test_staleness_survives_module_apply():
    """Module._apply (.double() / .float() / .to()) swaps parameters and buffers without registration
    hooks: the check must watch the new tensors, so a later in-place edit of a buffer (the positional
    table, BatchNorm running stats) is still seen."""
    m = _model().eval()
    v0 = m._version()
    m.double()
    v1 = m._version()
    assert v1 != v0
    pe = m.enc_embedding.position_embedding.pe
    assert pe.dtype == torch.float64
    with torch.no_grad():
        pe.add_(1.0)
    v2 = m._version()
    assert v2 != v1
    m.float()
    v3 = m._version()
    with torch.no_grad():
        dict(m.named_buffers())["encoder.encoders.0.conv_layers.0.norm.running_var"].mul_(2.0)
    assert m._version() != v3
