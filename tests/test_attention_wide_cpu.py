"""Heads wider than 128 (up to 256) construct; above 256 the model keeps refusing.  No GPU needed."""
import pytest


def test_head_dim_256_grouped_attention_constructs():
    from gaot_amd.model.layers.attn import GroupQueryFlashAttention
    attn = GroupQueryFlashAttention(512, 512, num_heads=2, num_kv_heads=1)
    assert attn.head_dim == 256
    shapes = {k: tuple(v.shape) for k, v in attn.named_parameters()}
    assert shapes == {"q_proj.weight": (512, 512), "k_proj.weight": (256, 512), "v_proj.weight": (256, 512),
                      "o_proj.weight": (512, 512)}


def test_hidden_2048_on_8_heads_transformer_constructs():
    """the 350 M point of the reference's throughput-against-size curve: hidden 2048 on the default 8 heads, head_dim 256"""
    from gaot_amd.model.layers.attn import Transformer, TransformerConfig
    cfg = TransformerConfig(hidden_size=2048)
    assert cfg.attn_config.num_heads == 8
    tf = Transformer(64, 64, cfg)
    heads = [m.head_dim for m in tf.modules() if hasattr(m, "head_dim") and hasattr(m, "q_proj")]
    assert heads and all(h == 256 for h in heads)


def test_head_dim_257_still_raises_and_names_the_bound():
    from gaot_amd.model.layers.attn import GroupQueryFlashAttention
    with pytest.raises(NotImplementedError, match="256"):
        GroupQueryFlashAttention(257, 257, num_heads=1, num_kv_heads=1)
