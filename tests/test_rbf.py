"""Radial-basis-function networks on the host: the oracle against the closed form on a network
written out by hand, ``NeuralEvaluator.rbf_layers`` on ``synth.rbf_pmml``, and every shape and limit
the RBF lowering refuses, by name."""

import math

import numpy as np
import pytest

from flink_jpmml_amd.bench import synth
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.plans import NotLowerable, lowering_dry_run

# width: h0 its own, h1 the layer's; altitude: h0 the network's (the layer has none), h1 its own
HAND = """<PMML xmlns="http://www.dmg.org/PMML-4_4" version="4.4"><Header/>
<DataDictionary><DataField name="f0" optype="continuous" dataType="double"/>
<DataField name="f1" optype="continuous" dataType="double"/><DataField name="y" optype="continuous" dataType="double"/>
</DataDictionary>
<NeuralNetwork functionName="regression" activationFunction="radialBasis" width="9" altitude="1.05">
<MiningSchema><MiningField name="y" usageType="target"/><MiningField name="f0"/><MiningField name="f1"/></MiningSchema>
<NeuralInputs>
<NeuralInput id="a"><DerivedField optype="continuous" dataType="double"><FieldRef field="f0"/></DerivedField></NeuralInput>
<NeuralInput id="b"><DerivedField optype="continuous" dataType="double"><FieldRef field="f1"/></DerivedField></NeuralInput>
</NeuralInputs>
<NeuralLayer width="1.5" normalizationMethod="simplemax">
<Neuron id="h0" width="0.75"><Con from="a" weight="1"/><Con from="b" weight="-2"/></Neuron>
<Neuron id="h1" altitude="0.9"><Con from="b" weight="0.5"/><Con from="a" weight="0.25"/></Neuron>
</NeuralLayer>
<NeuralLayer activationFunction="identity" normalizationMethod="none">
<Neuron id="o" bias="0.125"><Con from="h0" weight="2"/><Con from="h1" weight="-3"/></Neuron>
</NeuralLayer>
<NeuralOutputs><NeuralOutput outputNeuron="o"><DerivedField optype="continuous" dataType="double">
<FieldRef field="y"/></DerivedField></NeuralOutput></NeuralOutputs>
</NeuralNetwork></PMML>"""


def test_oracle_equals_the_closed_form_with_three_level_defaults():
    c = CompiledPmml.from_string(HAND)
    X = np.array([[0.3, -1.1], [1.0, -2.0], [2.5, 0.5]])
    got, valid = c.score_matrix_oracle(X)
    for (x0, x1), y in zip(X, got):
        a0 = math.exp(2 * math.log(1.05) - ((x0 - 1) ** 2 + (x1 + 2) ** 2) / (2 * 0.75 ** 2))
        a1 = math.exp(2 * math.log(0.9) - ((x0 - 0.25) ** 2 + (x1 - 0.5) ** 2) / (2 * 1.5 ** 2))
        assert y == pytest.approx(0.125 + (2 * a0 - 3 * a1) / (a0 + a1), rel=1e-14)
    assert valid.all()
    rbf = c.evaluator.rbf_layers()
    assert rbf["centers"].tolist() == [[1, -2], [0.25, 0.5]] and rbf["width"].tolist() == [0.75, 1.5]
    assert rbf["altitude"].tolist() == [1.05, 0.9] and rbf["fan_in"] == 2 and rbf["normalization"] == "simplemax"


def test_rbf_layers_round_trips_the_generator():
    c = CompiledPmml.from_string(synth.rbf_pmml(5, 7, 3, seed=2, classification=True, normalization="softmax",
                                                altitude=1.05))
    ev, rbf = c.evaluator, c.evaluator.rbf_layers()
    hidden, out = ev.nn.layers
    assert rbf["centers"].tolist() == [[w for _, w in n.connections] for n in hidden.neurons]
    own = [k % 3 == 0 for k in range(7)]
    assert rbf["width"].tolist() == [n.width if o else hidden.width for n, o in zip(hidden.neurons, own)]
    assert rbf["altitude"].tolist() == [n.altitude if o else 1.05 for n, o in zip(hidden.neurons, own)]
    assert all((n.width is not None) == o for n, o in zip(hidden.neurons, own))
    W, b, act, _, norm = rbf["output"]
    assert W.T.tolist() == [[w for _, w in n.connections] for n in out.neurons] and b.tolist() == [n.bias for n in out.neurons]
    assert (rbf["fan_in"], rbf["normalization"], act, norm) == (5, "softmax", "identity", "softmax")
    with lowering_dry_run():
        plan = c.plan("cpu")
    assert type(plan).__name__ == "RbfPlan" and (plan.kp, plan.n_tiles, plan.hidden_norm) == (16, 1, 1)


SMALL = synth.rbf_pmml(2, 2, 1, seed=0)
DENSE = '  <NeuralLayer activationFunction="identity"><Neuron id="z" bias="0"><Con from="o0" weight="1"/></Neuron></NeuralLayer>\n'
REFUSED = {
    "more than two layers": SMALL.replace("  <NeuralOutputs>", DENSE + "  <NeuralOutputs>").replace('outputNeuron="o0"', 'outputNeuron="z"'),
    "must be the first of two layers": SMALL.replace('activationFunction="identity"', 'activationFunction="radialBasis"'),
    "not connected to every input exactly once": SMALL.replace('<Con from="i1"', '<Con from="i0"', 1),
    "connection skips a layer": SMALL.replace('<Con from="h1"', '<Con from="i1"'),
    "width <= 0": SMALL.replace('<Neuron id="h0" width="', '<Neuron id="h0" width="-'),
    "altitude <= 0": lambda: synth.rbf_pmml(2, 2, 1, seed=0, altitude=0.0),
    "more than 128 inputs": lambda: synth.rbf_pmml(129, 1, 1, seed=0),
    "more than 1024 radialBasis units": lambda: synth.rbf_pmml(1, 1025, 1, seed=0),
    "more than 32 output neurons": lambda: synth.rbf_pmml(2, 2, 33, seed=0, classification=True),
    "A_max": lambda: synth.rbf_pmml(8, 2, 1, seed=0, altitude=2.0),
    "output activation": SMALL.replace('activationFunction="identity"', 'activationFunction="cube"'),
    "output normalisation": SMALL.replace('normalizationMethod="none"', 'normalizationMethod="max"'),
}


@pytest.mark.parametrize("reason", list(REFUSED))
def test_refused_shapes_and_limits_name_themselves(reason):
    doc = REFUSED[reason]
    c = CompiledPmml.from_string(doc() if callable(doc) else doc)
    with lowering_dry_run(), pytest.raises(NotLowerable, match=reason):
        c.plan("cpu")
