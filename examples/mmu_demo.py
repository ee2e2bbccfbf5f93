"""The w_clip_vit understanding flow of the reference's `inference_mmu.py` (lines 96-175) on the MI355X path:

    image -> CLIP ViT-L/14-336 tower (hidden_states[-2][:,1:]) -> mm_projector -> spliced between the embedded system prompt and the
    question -> mmu_vit visibility intervals -> prefill + KV-cached decode (greedy like the reference's top_k = 1, or --top-k / --temperature /
    --top-p, all drawn on the device)

Checkpoints / tokenizer are optional local directories; without them random-init weights of the true architecture and the
synthetic decimal-id tokenizer are used (same kernels, meaningless text).

    python examples/mmu_demo.py --max-new-tokens 32
    python examples/mmu_demo.py --top-k 0 --top-p 0.9 --temperature 0.8                                 # nucleus sampling
    python examples/mmu_demo.py --logprobs                                                              # + log-probability of every token
    python examples/mmu_demo.py --questions "What is in the image? *** What colour is it?"              # one prefill of the image prefix,
    python examples/mmu_demo.py --questions "What is in the image? *** What colour is it?" --follow-up  # every question appended to it
    python examples/mmu_demo.py --questions "q1 *** q2 *** ... (more than 8)" --share-prefix            # all decoded together on wide
                                                                                                        # slots that read the prefix in place

`--questions` takes the reference's ` *** ` separator (inference_mmu.py:86) and answers all of them from ONE `Showo.mmu_session`: the
607-row prefix (<|mmu|>, system prompt, <|soi|>, image, <|eoi|>) is prefilled once; each question is appended to its KV cache and the
session rewinds to the prefix for the next one.  `--follow-up` keeps the conversation instead: question 2 sees question 1 and its answer.
`--share-prefix` answers all questions in ONE `sess.generate_batch(..., slots=32, share_prefix=True)`: with more than 8 questions they
decode together on the slots of a wide batch, each slot holding only its question and answer and attending to the prefix in the
session's own cache (with 8 or fewer it is the plain generate_batch call).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import showo_amd  # noqa: E402
from showo_amd import synthetic  # noqa: E402
from showo_amd.clip_encoder import CLIP_VIT_L_14_336, CLIPVisionTower, vision_state_spec  # noqa: E402
from showo_amd.prompting_utils import UniversalPrompting, intervals_for_mmu_vit  # noqa: E402

SYSTEM_PROMPT_LEN = 28  # inference_mmu.py:36


def report_logprobs(lps):
    """--logprobs: the answer's log-likelihood, its per-token mean (log-perplexity) and the first values"""
    if lps is None:
        return
    v = lps.tolist()
    print(f"log-probabilities: sum {sum(v):.3f}, mean {sum(v) / len(v):.3f}:", [round(x, 3) for x in v[:24]], "..." if len(v) > 24 else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--showo", default=None, help="local Show-o (w_clip_vit) checkpoint directory")
    ap.add_argument("--clip", default=None, help="local openai/clip-vit-large-patch14-336 directory")
    ap.add_argument("--tokenizer", default=None)
    ap.add_argument("--image", default=None, help="image file (needs --clip with its preprocessor_config.json); default: noise")
    ap.add_argument("--question", default=None)
    ap.add_argument("--questions", default=None, help="several questions separated by ' *** ', answered from one mmu_session")
    ap.add_argument("--follow-up", action="store_true", help="with --questions: ask each question in the same conversation (no rewind)")
    ap.add_argument("--share-prefix", action="store_true",
                    help="with --questions: one generate_batch call on wide slots that share the prefix (slots=32, share_prefix=True)")
    ap.add_argument("--max-new-tokens", type=int, default=100)
    ap.add_argument("--top-k", type=int, default=1)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-p", type=float, default=None, help="nucleus sampling behind the top-k filter (needs --top-k other than 1; 0: no top-k)")
    ap.add_argument("--logprobs", action="store_true", help="also report every answer token's log-probability (return_logprobs=True)")
    ap.add_argument("--repetition-penalty", type=float, default=None,
                    help="penalise the tokens of the prompt's text ids and of the answer so far (Hugging Face's rule; 1: none)")
    ap.add_argument("--ban", default=None, help="comma-separated token ids (or, with --tokenizer, words) that must not be produced")
    ap.add_argument("--allow", default=None,
                    help="comma-separated token ids (or words) the answer is confined to, e.g. 'yes,no'; <eos> stays allowed")
    ap.add_argument("--no-repeat-ngram", type=int, default=None, help="no n-gram of this size may occur twice (1..16; no_repeat_ngram_size)")
    ap.add_argument("--min-new-tokens", type=int, default=None, help="<eos> is held back until the answer has this many tokens")
    ap.add_argument("--bad-words", default=None,
                    help="token-id sequences that must never be completed: ids separated by spaces, sequences by ';', e.g. '13 198;50256'")
    ap.add_argument("--stop", default=None, help="token-id sequences that end the answer, in the format of --bad-words, e.g. '198 198;13'")
    ap.add_argument("--num-beams", type=int, default=None, help="beam search with this many beams (2..8; greedy settings otherwise)")
    ap.add_argument("--length-penalty", type=float, default=1.0, help="with --num-beams: a hypothesis scores sum of log-probs / len ** this")
    ap.add_argument("--early-stopping", action="store_true", help="with --num-beams: stop once as many hypotheses are finished")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    rs = np.random.RandomState(a.seed)
    if a.tokenizer:
        from transformers import AutoTokenizer
        tok = AutoTokenizer.from_pretrained(a.tokenizer, padding_side="left")
        system, question = "A chat between a curious user and an artificial intelligence assistant.", a.question or "Describe the image."
    else:
        tok = synthetic.SyntheticTokenizer()
        system, question = synthetic.random_text(rs, SYSTEM_PROMPT_LEN), a.question or synthetic.random_text(rs, 24)

    def token_set(arg):
        """the ids of a --ban / --allow list: integers as they are, words through the tokenizer (every piece of the word)"""
        out = []
        for item in arg.split(","):
            item = item.strip()
            out += [int(item)] if item.lstrip("-").isdigit() else [int(t) for t in tok([item])["input_ids"][0]]
        return out

    uni = UniversalPrompting(tok, max_text_len=128, special_tokens=synthetic.SPECIAL_TOKENS, ignore_id=-100, cond_dropout_prob=0.1)
    if a.showo:
        model = showo_amd.Showo.from_pretrained(a.showo, max_batch=1, max_seq=1024)
    else:
        model = synthetic.random_init_showo(max_batch=1, max_seq=1024, w_clip_vit=True).eval()
    if a.clip:
        tower = CLIPVisionTower(a.clip, max_batch=1).cuda()
    else:
        spec = vision_state_spec(CLIP_VIT_L_14_336)
        sd = {k: torch.randn(shape) * (0.02 if len(shape) > 1 else 0.0) + (1.0 if k.endswith("norm.weight") or "layer_norm" in k and k.endswith("weight") else 0.0)
              for k, shape in spec.items()}
        tower = CLIPVisionTower("synthetic", config=CLIP_VIT_L_14_336, state_dict=sd, max_batch=1).cuda()
    if a.image and tower.image_processor is not None:
        from PIL import Image
        pixels = tower.image_processor.preprocess(Image.open(a.image).convert("RGB"), return_tensors="pt")["pixel_values"][0].cuda()
    else:
        pixels = torch.randn(3, 336, 336, device="cuda")
    sys_ids = tok([system])["input_ids"][0][:SYSTEM_PROMPT_LEN]
    q_ids = tok([question])["input_ids"][0]
    sp = uni.sptids_dict
    ids = torch.tensor([[int(sp['<|mmu|>'])] + sys_ids + [int(sp['<|soi|>']), int(sp['<|eoi|>'])] + q_ids], device="cuda")
    # logit adjustment (on the device, in front of every pick): only the keywords that were given are passed on
    adjust = {}
    if a.repetition_penalty is not None:
        adjust.update(repetition_penalty=a.repetition_penalty, repetition_context=ids[0])  # the prompt is embeddings: name its text ids
    if a.ban:
        adjust["banned_tokens"] = token_set(a.ban)
    if a.allow:
        adjust["allowed_tokens"] = token_set(a.allow) + ([int(tok.eos_token_id)] if tok.eos_token_id is not None else [])
    # sequence rules (the history is `repetition_context`, then the answer so far): only what was given is passed on
    id_seqs = lambda arg: [[int(t) for t in seq.split()] for seq in arg.split(";") if seq.strip()]
    if a.no_repeat_ngram is not None:
        adjust["no_repeat_ngram_size"] = a.no_repeat_ngram
    if a.min_new_tokens is not None:
        adjust["min_new_tokens"] = a.min_new_tokens
    if a.bad_words:
        adjust["bad_words_ids"] = id_seqs(a.bad_words)
    if a.stop:
        adjust["stop_sequences"] = id_seqs(a.stop)
    if a.num_beams is not None:  # (beam search on the device; it takes the greedy settings and no adjustment)
        adjust.update(num_beams=a.num_beams, length_penalty=a.length_penalty, early_stopping=a.early_stopping)
    with torch.no_grad():
        img_emb = model.mm_projector(tower(pixels[None]))                    # [1, 576, 2048]
        txt = model.showo.model.embed_tokens(ids)
        cut = 2 + len(sys_ids)                                               # after <|mmu|>, the system prompt and <|soi|>
        emb = torch.cat([txt[:, :cut], img_emb, txt[:, cut:]], dim=1)
        if a.questions:                                                      # one prefill of the prefix, no full-prompt call at all
            prefix = emb[:, :cut + img_emb.shape[1] + 1].contiguous()             # ... up to and including <|eoi|>
            sess = model.mmu_session(input_embeddings=prefix, attention_mask=intervals_for_mmu_vit(prefix, system_prompt_len=len(sys_ids)))
            start = sess.mark()
            if a.share_prefix:
                qs = [q.strip() for q in a.questions.split(" *** ")]
                q_embs = [model.showo.model.embed_tokens(torch.tensor([tok([q])["input_ids"][0]], device="cuda")) for q in qs]
                outs = sess.generate_batch(input_embeddings=q_embs, max_new_tokens=a.max_new_tokens, top_k=a.top_k, temperature=a.temperature,
                                           eot_token=tok.eos_token_id, top_p=a.top_p, return_logprobs=a.logprobs, slots=32, share_prefix=True,
                                           **adjust)
                outs, lpss = outs if a.logprobs else (outs, [None] * len(qs))
                for q, ans, lps in zip(qs, outs, lpss):
                    ans = [int(t) for t in ans]
                    print(f"[{sess.length} rows in the cache] {q!r} -> {len(ans)} tokens:", ans[:24], "..." if len(ans) > 24 else "")
                    report_logprobs(lps)
                    if a.tokenizer:
                        print(tok.decode(ans, skip_special_tokens=True))
                return
            for q in [q.strip() for q in a.questions.split(" *** ")]:
                q_emb = model.showo.model.embed_tokens(torch.tensor([tok([q])["input_ids"][0]], device="cuda"))
                ans = sess.generate(input_embeddings=q_emb, max_new_tokens=a.max_new_tokens, top_k=a.top_k, temperature=a.temperature,
                                    eot_token=tok.eos_token_id, top_p=a.top_p, return_logprobs=a.logprobs, **adjust)
                ans, lps = ans if a.logprobs else (ans, None)
                ans = [int(t) for t in ans]
                print(f"[{sess.length} rows in the cache] {q!r} -> {len(ans)} tokens:", ans[:24], "..." if len(ans) > 24 else "")
                report_logprobs(lps)
                if a.tokenizer:
                    print(tok.decode(ans, skip_special_tokens=True))
                if not a.follow_up:
                    sess.rewind(start)
            return
        mask = intervals_for_mmu_vit(emb, system_prompt_len=len(sys_ids))     # per-row intervals, no [1,1,L,L] tensor
        toks = model.mmu_generate(input_embeddings=emb, attention_mask=mask, max_new_tokens=a.max_new_tokens, top_k=a.top_k,
                                  temperature=a.temperature, eot_token=tok.eos_token_id, top_p=a.top_p, return_logprobs=a.logprobs,
                                  **adjust)
    toks, lps = toks if a.logprobs else (toks, None)
    out = [int(t) for t in toks]
    print(f"prompt of {emb.shape[1]} embeddings -> {len(out)} tokens:", out[:24], "..." if len(out) > 24 else "")
    report_logprobs(lps)
    if a.tokenizer:
        print(tok.decode(out, skip_special_tokens=True))


if __name__ == "__main__":
    main()
