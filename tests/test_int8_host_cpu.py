"""Host-side surface of precision 3 (int8 decode weights): no GPU needed."""
import os
import re

import pytest

import util


def test_set_precision_3_is_accepted_and_4_still_raises():
    d, _ = util.tiny_state()
    S = util.pkg().Showo
    m = S(False, d.vocab, d.llm_vocab, codebook_size=d.codebook, num_vq_tokens=d.num_vq_tokens, hidden_size=d.hidden,
          intermediate_size=d.ffn, num_hidden_layers=d.layers, num_attention_heads=d.heads)
    assert m.set_precision(3) is m and m._precision == 3
    with pytest.raises(ValueError, match="int8"):
        m.set_precision(4)
    assert m._precision == 3
    m.set_precision(0)


def test_quantization_module_imports():
    Q = util.pkg().quantization
    assert callable(Q.quantize_rows) and callable(Q.dequantize_rows)
    import showo_amd.quantization as Q2
    assert Q2 is Q


def test_header_declares_the_int8_symbols():
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    new = {"showo_quantize_rows_i8", "showo_dequantize_rows_i8", "showo_engine_load_q8"}
    assert new <= declared
    assert new <= set(util.lib().EXPORTED_SYMBOLS)
