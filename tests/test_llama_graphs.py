"""Every graph LlamaDecoder can build without a device, against its recorded signature
(tests/golden/llama_graphs.json, tests/llama_graph_sig.py): the token graph with either rope
source, both ranks of a two-way row split in both modes (with the nodes behind dec.gathers and
dec.reduces), the prompt graph of one and of several tokens, and the batch graph. Node for node:
op, shape, op_params, flags, operand order, which node or leaf each operand is, and which storage
at which offset each leaf points into. Host only."""
import json
import os

import pytest

from tests import llama_graph_sig as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llama_graphs.json")
NAMES = ["token.row", "token.table", "split.gather.0", "split.gather.1", "split.reduce.0", "split.reduce.1",
         "prompt.1", "prompt.5", "batch.3.32"]
N_NODES = [34, 34, 43, 43, 39, 35, 34, 36, 34]


@pytest.fixture(scope="module")
def built():
    return S.graphs()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_graph_is_recorded(built, golden):
    assert sorted(built) == sorted(golden) == sorted(NAMES)
    assert [len(golden[k]["nodes"]) for k in NAMES] == N_NODES


@pytest.mark.parametrize("name", NAMES)
def test_graph_matches_recorded_signature(built, golden, name):
    got, want = built[name], golden[name]
    assert len(got["nodes"]) == len(want["nodes"])
    for i, (a, b) in enumerate(zip(got["nodes"], want["nodes"])):
        assert a == b, (name, i, a, b)
    assert sorted(got) == sorted(want)
    if name.startswith("split."):
        assert got["gathers"] == want["gathers"]
        assert got["reduces"] == want["reduces"]
        n_g, n_r = (9, 0) if ".gather." in name else (1, 4)
        assert (len(want["gathers"]), len(want["reduces"])) == (n_g, n_r)
