"""Records tests/golden/masked_generate.pt: the REFERENCE's greedy decode of a left-padded batch.

The reference's LLaMA is driven the way HF's generation loop would drive it for a padded batch: its own
`LlamaForCausalLM.forward` with the attention mask, its own `prepare_inputs_for_generation` (position_ids =
cumsum(mask) - 1, the mask extended by a one per step) and its own `past_key_values`, on micro_all's weights and
embeddings, for 8 tokens.  tests/test_decode_ragged_cpu.py asserts that the restated masked loop (oracle.restate)
reproduces the recorded per-step logits and ids; generate(attention_mask=) is then tested against that restatement.

Needs the reference tree (oracle.ref_loader); the test reads only the committed fixture.

    python scripts/make_golden_masked_generate.py
"""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import GOLDEN_DIR, load_case  # noqa: E402
from oracle import configs, ref_loader  # noqa: E402

NEW_TOKENS = 8


def left_mask(B, S0):
    mask = torch.ones((B, S0), dtype=torch.long)
    mask[1, :5] = 0
    return mask


def cached(llm, emb, mask, steps):
    """the reference's cached forward under the mask; appends each step's last-row logits to `steps`"""
    step = llm.prepare_inputs_for_generation(None, attention_mask=mask, inputs_embeds=emb, use_cache=True)
    out = llm(**step)
    ids = []
    for _ in range(NEW_TOKENS):
        steps.append(out.logits[:, -1, :].detach().clone())
        nxt = out.logits[:, -1, :].argmax(-1)
        ids.append(nxt)
        mask = torch.cat([mask, torch.ones((mask.shape[0], 1), dtype=mask.dtype)], dim=1)
        step = llm.prepare_inputs_for_generation(nxt.unsqueeze(1), past_key_values=out.past_key_values,
                                                 attention_mask=mask, use_cache=True)
        out = llm(**step)
    return torch.stack(ids, dim=1)


def uncached(llm, emb, mask, steps):
    """the fallback: the reference's uncached forward with attention_mask and position_ids, the prefix recomputed"""
    E = llm.get_input_embeddings().weight
    ids = []
    for _ in range(NEW_TOKENS):
        pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)
        out = llm(inputs_embeds=emb, attention_mask=mask, position_ids=pos)
        steps.append(out.logits[:, -1, :].detach().clone())
        nxt = out.logits[:, -1, :].argmax(-1)
        ids.append(nxt)
        emb = torch.cat([emb, torch.nn.functional.embedding(nxt, E).unsqueeze(1)], dim=1)
        mask = torch.cat([mask, torch.ones((mask.shape[0], 1), dtype=mask.dtype)], dim=1)
    return torch.stack(ids, dim=1)


def main():
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = ref_loader.build_reference_model(cfg, seed=fx["seed"])
    sd = model.state_dict()
    for k, v in fx["state"].items():
        if k.startswith("llm.") and not torch.equal(sd[k], v):
            raise SystemExit(f"{k}: the reference at seed {fx['seed']} does not hold micro_all's committed weights")
    emb = fx["inputs_embeds"]
    mask = left_mask(*emb.shape[:2])
    with torch.no_grad():
        steps = []
        try:
            ids = cached(model.llm, emb, mask, steps)
            source = ("reference LlamaForCausalLM.forward with attention_mask, its prepare_inputs_for_generation and "
                      "its past_key_values (cached)")
        except Exception as e:  # noqa: BLE001  (the installed transformers may not let the cached forward take the mask)
            steps = []
            ids = uncached(model.llm, emb, mask, steps)
            source = ("reference LlamaForCausalLM.forward UNCACHED with attention_mask and position_ids = cumsum - 1 "
                      f"(its cached forward refused the mask: {type(e).__name__}: {str(e)[:120]})")
    out = dict(config_name=fx["config_name"], seed=fx["seed"], state_file=fx["state_file"], mask=mask, ids=ids,
               step_logits=torch.stack(steps, dim=1), source=source)
    path = os.path.join(GOLDEN_DIR, "masked_generate.pt")
    torch.save(out, path)
    print(f"{path}: ids {ids.tolist()}\n  {source}")


if __name__ == "__main__":
    main()
