"""GRU widths other than 128 on the host side: the model parser's rule (units per direction in UNITS_ACCEPTED, one width
for every GRU layer of a model), the architectures and weight makers at a given width, and the flat parameter layout that
include/poreover_hip.h documents.  No device."""
import json

import numpy as np
import pytest

ARCHS = ["bigru3", "conv1_bigru3", "conv2_bigru3", "conv1_gru5"]
WIDTHS = [16, 32, 48, 64, 80, 96, 112, 128]
GRU_KINDS = ("bigru", "gru", "gru_back")


def test_accepted_widths():
    from poreover_amd.network import checkpoint as C
    assert list(C.UNITS_ACCEPTED) == WIDTHS and C.UNITS == 128


@pytest.mark.parametrize("units", WIDTHS)
@pytest.mark.parametrize("arch", ARCHS)
def test_every_architecture_parses_at_every_width(arch, units):
    from poreover_amd.network import checkpoint as C
    spec = C.parse_model_json(json.dumps(C.architecture(arch, units=units)))
    assert [k for k, _ in spec] == [k for k, _ in C.parse_model_json(C.ARCHITECTURES[arch]())]
    gru = [s for k, s in spec if k in GRU_KINDS]
    assert len(gru) == (5 if arch == "conv1_gru5" else 3) and all(s["units"] == units for s in gru)


def _with_units(arch, layer, units):
    """the architecture at 128 units with one GRU layer (index into the Keras layer list) at `units`"""
    from poreover_amd.network import checkpoint as C
    cfg = C.architecture(arch)
    c = cfg["config"]["layers"][layer]["config"]
    (c["layer"]["config"] if "layer" in c else c)["units"] = units
    return cfg


@pytest.mark.parametrize("units", [0, 8, 24, 144, 256])
@pytest.mark.parametrize("arch", ["conv1_bigru3", "conv1_gru5"])
def test_widths_outside_the_set_refused(arch, units):
    from poreover_amd.network import checkpoint as C
    cfg = C.architecture(arch)
    for ly in cfg["config"]["layers"]:      # every GRU layer at the refused width: the width is what is wrong, not a mix
        c = ly["config"]
        if ly["class_name"] == "Bidirectional":
            c["layer"]["config"]["units"] = units
        elif ly["class_name"] == "GRU":
            c["units"] = units
    with pytest.raises(C.NetworkError, match="units") as e:
        C.parse_model_json(cfg)
    assert "16, 32, 48, 64, 80, 96, 112, 128" in str(e.value) and "%d units" % units in str(e.value)
    with pytest.raises(C.NetworkError, match="units"):
        C.synthetic_weights(cfg)


@pytest.mark.parametrize("arch,layer,units", [("conv1_bigru3", 1, 64), ("conv1_bigru3", 3, 64), ("conv1_gru5", 3, 32),
                                              ("conv1_gru5", 1, 32)])
def test_layers_of_different_widths_refused(arch, layer, units):
    from poreover_amd.network import checkpoint as C
    with pytest.raises(C.NetworkError, match="units") as e:
        C.parse_model_json(_with_units(arch, layer, units))
    assert "16, 32, 48, 64, 80, 96, 112, 128" in str(e.value)
    assert "%d" % units in str(e.value) and "128" in str(e.value)


def test_backward_layer_of_another_width_refused():
    from poreover_amd.network import checkpoint as C
    cfg = C.architecture("bigru3", units=48)
    c = cfg["config"]["layers"][1]["config"]
    c["backward_layer"] = json.loads(json.dumps(c["layer"]))
    c["backward_layer"]["config"]["units"] = 64
    with pytest.raises(C.NetworkError, match="backward layer has 64 units"):
        C.parse_model_json(cfg)
    c["backward_layer"]["config"]["units"] = 48
    assert [s.get("units") for _, s in C.parse_model_json(cfg)] == [48, 48, 48, None]


def _params(arch, H, K=9, F=24):
    """the parameter count of include/poreover_hip.h's layout: Conv1D K·cin·F + F; a GRU direction cin·3H + H·3H + 2·3H;
    Dense cin·5 + 5"""
    G = 3 * H
    conv = {"bigru3": 0, "conv1_bigru3": 1, "conv2_bigru3": 2, "conv1_gru5": 1}[arch]
    n, cin = 0, 1
    for _ in range(conv):
        n += K * cin * F + F
        cin = F
    nd = 1 if arch == "conv1_gru5" else 2
    for _ in range(5 if arch == "conv1_gru5" else 3):
        n += nd * (cin * G + H * G + 2 * G)
        cin = nd * H
    return n + cin * 5 + 5


@pytest.mark.parametrize("maker", ["synthetic", "init"])
@pytest.mark.parametrize("arch", ARCHS)
def test_weights_and_network_at_48_units(arch, maker):
    from poreover_amd.network import checkpoint as C
    from poreover_amd.network.train import init_weights
    cfg = C.architecture(arch, kernel_size=9, filters=24, units=48)
    w = C.synthetic_weights(cfg, seed=1) if maker == "synthetic" else init_weights(cfg, 1)
    net = C.load_network(w, cfg)
    cin = {"bigru3": 1}.get(arch, 24)
    for l in net.layers:
        if l.kind not in GRU_KINDS:
            continue
        nd = 2 if l.kind == "bigru" else 1
        assert l.cin == cin and l.cout == 48 * nd and len(l.tensors) == 3 * nd
        for d in range(nd):
            assert [t.shape for t in l.tensors[3 * d:3 * d + 3]] == [(cin, 144), (48, 144), (2, 144)]
        cin = l.cout
    assert net.layers[-1].cin == cin
    assert net.n_params() == net.flat_weights().size == _params(arch, 48)
    if maker == "init":
        for l in net.layers:
            for u in l.tensors[1::3] if l.kind in GRU_KINDS else []:
                # Keras' Orthogonal on (48, 144), as tests/test_train_cpu.py checks it at (128, 384): orthonormal rows,
                # U·Uᵀ = I (48 x 48) — the three gate blocks' B·Bᵀ sum to I, each alone is not orthogonal
                assert np.abs(u.astype(np.float64) @ u.astype(np.float64).T - np.eye(48)).max() <= 1e-6


@pytest.mark.parametrize("units", [16, 112])
def test_parameter_count_matches_the_documented_layout(units):
    from poreover_amd.network import checkpoint as C
    for arch in ARCHS:
        cfg = C.architecture(arch, filters=24, units=units)
        assert C.load_network(C.synthetic_weights(cfg, seed=0), cfg).n_params() == _params(arch, units)
    # and the known count at the default width
    assert C.load_network(C.synthetic_weights(C.architecture("conv1_bigru3"), seed=0)).n_params() == 893189


def test_fan_in_fallback_uses_the_model_width():
    """without role statistics a tensor is N(0, 1 / fan_in): the recurrent kernel's deviation follows H"""
    from poreover_amd.network import checkpoint as C
    v = "layer_with_weights-1/forward_layer/cell/recurrent_kernel/.ATTRIBUTES/VARIABLE_VALUE"
    for units in (16, 64):
        w = C.synthetic_weights(C.architecture("conv1_bigru3", filters=24, units=units), seed=2)
        assert w[v].shape == (units, 3 * units)
        assert abs(float(w[v].std()) * np.sqrt(units) - 1.0) < 0.1


def test_npz_round_trip_at_48_units(tmp_path):
    from poreover_amd.network import checkpoint as C
    cfg = C.architecture("conv1_gru5", filters=24, units=48)
    net = C.load_network(C.synthetic_weights(cfg, seed=3), cfg)
    path = C.write_weights(str(tmp_path / "small"), net)
    assert path.endswith(".npz")
    back = C.load_network(path, cfg)
    assert np.array_equal(back.flat_weights().view(np.uint32), net.flat_weights().view(np.uint32))
    # the weights do not fit the default 128-unit model
    with pytest.raises(C.NetworkError, match="shape"):
        C.load_network(path, C.architecture("conv1_gru5", filters=24))


def test_default_width_is_unchanged():
    """architecture() without units is the 128-unit model of ARCHITECTURES, and the makers draw the same values for it"""
    from poreover_amd.network import checkpoint as C
    for arch in ARCHS:
        assert C.architecture(arch) == C.ARCHITECTURES[arch]() == C.architecture(arch, units=128)
