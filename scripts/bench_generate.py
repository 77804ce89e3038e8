"""Greedy generate() throughput (KV-cache path), LLaMA-7B bf16, image + audio + 128-token prompt."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from macaw_llm_amd.factory import baseline_config, build_model, synthetic_inputs
dev = torch.device("cuda:0")
cfg = baseline_config("real_7b")
model = build_model(cfg, dtype=torch.bfloat16, device=dev, seed=1).eval()
# warm-up (allocator pools, kernel attributes) so that the first measured batch size is not inflated
_w = synthetic_inputs(cfg, 1, 128, modalities=("images", "audios"), seed=2, device=dev)
with torch.no_grad():
    model.llm.generate(inputs_embeds=model.prepare_inputs_for_generation(_w)[0], max_new_tokens=4, eos_token_id=-1)
# usage: bench_generate.py [B ...]; BG_SKINNY32="19,22" repeats every batch size > 16 with each kernel for
# 17 ... 32 token rows (MK_GEMM_SKINNY32, read per call by csrc/gemm.hip: one process and one model serve all variants)
#        bench_generate.py --fp8-ab [--reps R] [B ...]: every batch size with decode_weights=None and "fp8" in THIS process
# on THIS model, alternated bf16 / fp8 / bf16 / fp8 ... (R repetitions each, default 3): ms per token of every run, the
# medians, their ratio, the bf16 run-to-run spread (a difference counts only beyond it) and the achieved weight-stream
# bandwidth of each mode (fp8 bytes: half the projections' plus f32[N] scales)
#        bench_generate.py --kv8-ab [--prompt-tokens N] [--reps R] [B ...]: the same alternation for kv_cache=None / "fp8" (the
# e4m3 KV cache), with the KV bytes a decode step reads in each mode at the middle of the timed window; --prompt-tokens N
# replaces the 128 text tokens of the prompt (the image and audio prefixes stay), e.g. 1900 for a context near 2048
#        bench_generate.py --sample-ab [--reps R] [B ...]: greedy against do_sample=True, top_k=50, top_p=0.9 (seed 1), alternated
# the same way: ms per token of every run, the medians, their difference and the greedy run-to-run spread (the difference
# counts only beyond it), then the stand-alone time of one ops.sample_rows launch against ops.argmax_rows on [B, 32000] logits
#        bench_generate.py --ragged-ab [--prompt-tokens N] [--short-tokens M] [--reps R] [B ...]: a LEFT-PADDED batch (default
# B = 32) whose text lengths fall linearly from N (default 1900) to M (default 150), once with attention_mask= (the compacted,
# ragged KV cache: a step streams the sum of the real lengths) and once as today's call without a mask (every sample streams
# all S0 rows and attends to its pad tokens), alternated the same way, with the KV bytes a step reads in each mode
#        bench_generate.py --mxfp4-ab [--reps R] [B ...]: the --fp8-ab alternation over THREE modes, bf16 / fp8 / mxfp4 (default
# B = 1 8 16 32, R = 5): the bytes each mode streams per token (mxfp4: codes + E8M0 exponents of the layers' projections, the
# e4m3 lm_head with its f32 scales), ms per token of every run, the medians, the implied bandwidth, the ratios and the
# run-to-run spread of every mode (a difference counts only beyond the spreads)
#        bench_generate.py --beam-ab [--reps R]: greedy at batch B * K against num_beams=K at batch B for (B, K) = (1, 4), (8, 4),
# (2, 16) -- the same number of token rows per step -- alternated the same way: ms per token of every run, the medians,
# their difference and the greedy run-to-run spread, then the stand-alone time of one ops.beam_emit launch against
# ops.decode_emit on [B * K, 32000] logits
#        bench_generate.py --processors-ab [--reps R] [B ...]: greedy against repetition_penalty=1.2, no_repeat_ngram_size=3,
# min_new_tokens=8 (the logits processors, one ops.logits_process launch in front of the emit of every step), alternated the
# same way: ms per token of every run, the medians, their difference and the greedy run-to-run spread (the difference counts
# only beyond it), then the stand-alone time of one ops.logits_process launch against ops.decode_emit on [B, 32000] logits
# with a history of 200 prompt + 100 generated ids
#        bench_generate.py --lookup-ab [--reps R]: greedy against prompt_lookup_num_tokens=7 (prompt-lookup speculative decoding)
# at batch 1, alternated the same way, over two histories: "accepting" = the greedy output itself handed in as input_ids (the
# drafts are the answer: an upper bound) and "cold" = no input_ids (the history is the generated tokens only: the price of the
# 8-row verify step wherever the output does not repeat itself).  ms per EMITTED token of every run, tokens per verify step,
# the medians, lookup / greedy and the run-to-run spread of each arm
#        bench_generate.py --logprobs-ab [--reps R] [B ...]: greedy against return_logprobs=True and return_logprobs=True,
# top_logprobs=5 (one ops.decode_emit_logprobs launch behind the emit of every step), alternated the same way: ms per token of
# every run, the medians, their differences to greedy and the greedy run-to-run spread (a difference counts only beyond it), then
# the stand-alone time of one ops.token_logprobs / ops.decode_emit_logprobs launch (n = 0, 5, 20) against ops.argmax_rows and
# ops.decode_emit on [B, 32000] logits
#        bench_generate.py --cfg-ab [--reps R] [B ...]: classifier-free guidance (default B = 1, 8, 16).  Three arms alternated
# the same way: greedy at batch B, greedy at batch 2B (the token rows of the guided call) and guidance_scale=1.5 at batch B with
# the text-only prompt as the negative one (another length: the padded-batch path at 2B rows).  ms per token of every run, the
# medians, guided - greedy(2B) and guided - greedy(B), the greedy run-to-run spreads, then the stand-alone time of one
# ops.cfg_combine launch on [2B, 32000] logits against ops.decode_emit_logprobs (n = 0) and one embedding gather
#        bench_generate.py --stop-ab [--reps R] [B ...]: greedy against stop_sequences (4 sequences) plus bad_words_ids (4
# sequences) that never fire -- ids above the model's vocabulary V (the lm_head's rows), which it cannot emit -- so both arms run
# the same 72 tokens and the difference is the two launches per step (ops.seq_ban in front of the emit, ops.stop_match behind
# it), alternated the same way: ms per token of every run, the medians, their difference and the greedy run-to-run spread (the
# difference counts only beyond it).  A third arm times the 72-token call alone with every sample stopping on a sequence at its
# LAST column (each row's own last ids; skipped where a row's ids repeat so that it would stop earlier): against the never-fire
# call of 72 tokens the difference is the search for the returned width behind the loop (one ops.stop_match launch per column).
# Then the stand-alone time of one ops.seq_ban / ops.stop_match launch (tables of 4 and of 1000 sequences) against
# ops.decode_emit on [B, V] logits with 100 generated ids
#        bench_generate.py --warpers-ab [--reps R] [B ...]: four arms alternated in one process -- greedy; do_sample=True, top_k=50,
#            top_p=0.9 (--sample-ab's sampled arm); that plus min_p=0.05; that plus typical_p=0.9, epsilon_cutoff=3e-4,
#            eta_cutoff=2e-3 -- ms / token per arm with each arm's run-to-run spread, and the emit launch of each arm by itself
#        bench_generate.py --nsample-ab [--prompt-tokens N] [--reps R]: parallel sampling for (B, n) = (1, 4), (2, 16), (8, 4).
# Three arms alternated in this process on this model, all with do_sample=True, top_k=50, top_p=0.9, seed 1: "repeat" = the
# prompts repeated n times, a batch of B * n (today's way); "shared R=1" = num_samples=n at batch B (the prompt cache stored once,
# ops.decode_step_attn_shared) under MK_SHARED_ATTN_ROWS=1, one workgroup per row; "shared R=4" = the same under
# MK_SHARED_ATTN_ROWS=4, four rows of a prompt one after the other in one workgroup (the variable is read at every call, and the
# step is captured anew by every generate() call).  ms per token of every run, the medians and each arm's run-to-run spread, the time to the first
# token (the call with max_new_tokens=1: prefill + token 0), and the KV bytes each arm allocates for the 72-token call (from the
# shapes, and the allocator's peak over the call)
#        bench_generate.py --session-ab [--prompt-tokens N] [--reps R] [B ...]: a second turn over a kept KV cache (default
# B = 1, 8; N = 1900: a 1916-row first prompt).  Turn 1 = the image + audio + text prompt plus 64 new tokens; turn 2 = 32 prompt
# tokens plus new tokens.  Two arms alternated in this process on this model: "session" = generate(session=s) on the session
# turn 1 returned (a fresh, untimed turn 1 in front of every timed call: a call advances its session) and "fresh" = today's only
# way, one call on the concatenated history [turn 1's prompt | its 64 tokens | turn 2's prompt].  Time to the first token of
# turn 2 (the call with max_new_tokens=1) and ms per token ((72 - 8 tokens) / 64), each with its run-to-run spread; then what a
# follow-up turn through MM_LLMs skips on top: the towers and the alignment (prepare_inputs_for_generation), timed alone
#        bench_generate.py --adapters-ab [--reps R] [B ...]: mixed-adapter LoRA decoding (default B = 1, 8, 32), r = 16 on all seven
# projections.  Four greedy arms alternated in this process on this model: "base" = no adapter; "merged" = today's single-adapter
# call, a live adapter that generate() merges into temporary copies of the weights; "names x1" = adapter_names with one adapter
# for every row; "names x4" = adapter_names cycling over four distinct adapters (and the same rows through the mk_lora_bgmv
# kernels: 8 more launches per layer and token, 256 for the model).  ms per token of every run ((72 - 8 tokens) / 64), the
# medians and each arm's run-to-run spread, and the time to the first token (the call with max_new_tokens=1: for "merged" it
# holds the merge, for the names arms the prefill's per-run adapter launches)
#        bench_generate.py --grammar-ab [--reps R] [B ...]: grammar-constrained decoding (default B = 1, 8, 32).  Three greedy arms
# alternated in this process on this model: "greedy" = no grammar; "free" = a one-state grammar that allows every token, so the
# ids are the greedy ones and the difference is the two launches per step (ops.grammar_mask in front of the emit,
# ops.grammar_advance behind it); "json" = the 35-state pattern \{"name": "[a-z ]{1,12}", "n": (0|[1-9]\d?)\} over a synthetic
# vocabulary of the model's size (3 specials, the 256 bytes, random pieces of 2 to 17 bytes), whose answer ends by itself: every
# free arm is timed against greedy over 72 tokens ((72 - 8 tokens) / 64) and the json arm against greedy over its own width W ((W - 8 tokens) / (W - 8); 3 in place of 8 where W <= 16), ms per token of every run, the medians, the
# differences and the greedy run-to-run spread.  Then the time of one ops.grammar_mask and one ops.grammar_advance launch inside a
# hipGraph against their neighbours ops.decode_emit, ops.seq_ban and ops.stop_match, and the making of a table (ops.grammar_build plus the trim) for (S, V) = (35, V) and for a pattern of 3001
# states
#        bench_generate.py --score-ab [--prompt-tokens N] [--reps R] [B ...]: score() of n = 4 given answers of 16 tokens per
# prompt (default B = 1, 8).  Three arms alternated in this process on this model: "score" = score() (one prefill per prompt,
# token 0 at B rows, then the B * n * 15 fed rows as one GEMM pass over the prompt cache: ops.score_attn); "recompute" =
# score(use_cache=False), the prompt recomputed per option ([prompt | option] as a padded batch of B * n); "steps" = what
# teacher-forced decode steps would cost: generate()'s ms per token at batch B * n ((72 - 8 tokens) / 64, greedy) x 16.  ms per
# call of every run, the medians, each arm's run-to-run spread and the ratios; the towers and the alignment
# (prepare_inputs_for_generation) run once per prompt outside every arm and are timed alone
#        bench_generate.py --penalties-ab [--reps R] [B ...]: the per-request penalties (default B = 1, 8, 32).  Three greedy arms
# alternated in this process on this model: "greedy"; "penalties" = frequency_penalty=0.5, presence_penalty=0.5; "+bias" = the
# same plus a 300-entry logit_bias (one ops.logits_penalize launch in front of the emit of every step): ms per token of every
# run ((72 - 8 tokens) / 64), the medians, the differences to greedy and the greedy run-to-run spread (a difference counts only
# beyond it).  Then the time of one ops.logits_penalize launch inside a hipGraph at n = 0 and at n = 2048 generated ids (what
# the counting costs at the long end), with and without the 300-entry bias, against ops.decode_emit and ops.logits_process
#        bench_generate.py --params-ab [--reps R] [B ...]: per-request sampling (default B = 1, 8, 32).  Three sampled arms
# alternated in this process on this model: "scalar" = do_sample=True, top_k=50, top_p=0.9 (seed 1); "table" = sampling_params
# with that dict on every row (ops.decode_emit_sample_table in place of ops.decode_emit_sample: the same work plus one small
# uniform load per workgroup); "mixed" = the same list with every second row greedy.  ms per token of every run ((72 - 8 tokens)
# / 64), the medians, each table arm's difference to the scalar arm and the scalar arm's run-to-run spread, which is the yardstick
PARAMS = "--params-ab" in sys.argv
PENALTIES = "--penalties-ab" in sys.argv
SCORE = "--score-ab" in sys.argv
GRAMMAR = "--grammar-ab" in sys.argv
ADAPTERS = "--adapters-ab" in sys.argv
SESSION = "--session-ab" in sys.argv
NSAMPLE = "--nsample-ab" in sys.argv
STOP = "--stop-ab" in sys.argv
CFG = "--cfg-ab" in sys.argv
LOGPROBS = "--logprobs-ab" in sys.argv
LOOKUP = "--lookup-ab" in sys.argv
AB = "--fp8-ab" in sys.argv
PROC = "--processors-ab" in sys.argv
BEAM = "--beam-ab" in sys.argv
MX4 = "--mxfp4-ab" in sys.argv
RAGGED = "--ragged-ab" in sys.argv
SAMPLE = "--sample-ab" in sys.argv
WARPERS = "--warpers-ab" in sys.argv
KV8 = "--kv8-ab" in sys.argv
_VAL = ("--reps", "--prompt-tokens", "--short-tokens")
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else (5 if "--mxfp4-ab" in sys.argv else 3)
PROMPT = int(sys.argv[sys.argv.index("--prompt-tokens") + 1]) if "--prompt-tokens" in sys.argv else (1900 if RAGGED or SESSION else 128)
SHORT = int(sys.argv[sys.argv.index("--short-tokens") + 1]) if "--short-tokens" in sys.argv else 150
_args = [a for i, a in enumerate(sys.argv[1:], 1) if a not in ("--fp8-ab", "--mxfp4-ab", "--kv8-ab", "--sample-ab", "--ragged-ab", "--beam-ab", "--processors-ab", "--lookup-ab", "--logprobs-ab", "--cfg-ab", "--stop-ab", "--nsample-ab", "--session-ab", "--adapters-ab", "--grammar-ab", "--score-ab", "--warpers-ab", "--penalties-ab", "--params-ab", *_VAL) and sys.argv[i - 1] not in _VAL]
if PARAMS:
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    D = dict(top_k=50, top_p=0.9, seed=1)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ARMS = {"scalar": dict(do_sample=True, **D), "table": dict(sampling_params=[D] * B),
                "mixed": dict(sampling_params=[None if b % 2 else D for b in range(B)])}
        ms = {a: [] for a in ARMS}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            gen = lambda arm, new: model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, pad_token_id=0, **ARMS[arm])  # noqa: E731
            for arm in ARMS:
                gen(arm, 8)                         # warm-up of every arm
            for rep in range(REPS):
                for arm in ARMS:
                    t = {}
                    for new in (8, 72):
                        ids, t[new] = timed(lambda: gen(arm, new))
                        assert ids.shape[1] == new
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {arm:6s}: decode {ms[arm][-1]:6.3f} ms/token over 64 tokens", flush=True)
        spread = max(ms["scalar"]) - min(ms["scalar"])
        for arm in ("table", "mixed"):
            d = med(ms[arm]) - med(ms["scalar"])
            print(f"B={B:2d}: scalar {med(ms['scalar']):6.3f} ms/token, {arm} {med(ms[arm]):6.3f} ms/token (spread "
                  f"{(max(ms[arm]) - min(ms[arm])) * 1e3:6.1f} us), {arm} - scalar = {d * 1e3:+7.1f} us per token "
                  f"({d / med(ms['scalar']) * 100:+5.2f} %), scalar run-to-run spread {spread * 1e3:6.1f} us: "
                  f"{'inside' if abs(d) <= spread else 'OUTSIDE'} the spread", flush=True)
    sys.exit(0)
if PENALTIES:
    from macaw_llm_amd import ops
    V = model.llm.lm_head.weight.shape[0]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    g = torch.Generator().manual_seed(5)
    BIAS = {int(c): float(v) for c, v in zip(torch.randperm(V, generator=g)[:300], torch.rand(300, generator=g) * 10 - 5)}
    ARMS = {"greedy": {}, "penalties": dict(frequency_penalty=0.5, presence_penalty=0.5),
            "+bias": dict(frequency_penalty=0.5, presence_penalty=0.5, logit_bias=BIAS)}

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {a: [] for a in ARMS}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            gen = lambda arm, new: model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, pad_token_id=0, **ARMS[arm])  # noqa: E731
            for arm in ARMS:
                gen(arm, 8)                         # warm-up of every arm
            for rep in range(REPS):
                for arm in ARMS:
                    t = {}
                    for new in (8, 72):
                        ids, t[new] = timed(lambda: gen(arm, new))
                        assert ids.shape[1] == new
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {arm:9s}: decode {ms[arm][-1]:6.3f} ms/token over 64 tokens", flush=True)
        spread = max(ms["greedy"]) - min(ms["greedy"])
        for arm in ("penalties", "+bias"):
            d = med(ms[arm]) - med(ms["greedy"])
            print(f"B={B:2d}: greedy {med(ms['greedy']):6.3f} ms/token, {arm} {med(ms[arm]):6.3f} ms/token, {arm} - greedy = "
                  f"{d * 1e3:+7.1f} us per token ({d / med(ms['greedy']) * 100:+5.2f} %), greedy run-to-run spread "
                  f"{spread * 1e3:6.1f} us: {'inside' if abs(d) <= spread else 'OUTSIDE'} the spread", flush=True)
        # one launch by itself: 40 launches captured in a hipGraph (no host between them), replayed 4 times between two events.
        # f = p = 2^-20: the 160 launches rewrite the same columns without ever driving a bf16 logit away
        x = torch.randn(B, V, device=dev).mul_(3).to(torch.bfloat16)
        out = torch.randint(3, V, (B, 2048), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
        tok, done = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.bool, device=dev)
        out_e = torch.zeros((B, 256), dtype=torch.long, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        f = torch.full((B,), 2.0 ** -20, dtype=torch.float32, device=dev)
        tab = ops.BiasTable({c: 2.0 ** -20 for c in BIAS}, B, V, dev)
        n0, n2k = (torch.tensor([n], dtype=torch.int32, device=dev) for n in (0, 2048))
        us = {}
        for name, fn in (("decode_emit", lambda: ops.decode_emit(x, V, 0, -1, tok, done, out_e, st)),
                         ("logits_process n=2048 (theta 1.0001)", lambda: ops.logits_process(x, V, out, n2k, 0, repetition_penalty=1.0001)),
                         ("logits_penalize n=0 bias", lambda: ops.logits_penalize(x, V, out, n0, 0, f, f, tab)),
                         ("logits_penalize n=100", lambda: ops.logits_penalize(x, V, out, n0, 100, f, f)),
                         ("logits_penalize n=2048", lambda: ops.logits_penalize(x, V, out, n2k, 0, f, f)),
                         ("logits_penalize n=2048 bias", lambda: ops.logits_penalize(x, V, out, n2k, 0, f, f, tab))):
            for i in range(5):
                fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(40):
                    fn()
            graph.replay()
            st.zero_()                              # (the emit's output column: 5 + 5 * 40 launches stay inside out_e's 256)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(4):
                graph.replay()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 160 * 1e3
            st.zero_()
            del graph
        print(f"B={B:2d}: one launch on [B, {V}] bf16 logits, 40 in a hipGraph (device time incl. the gap between two graph nodes): " +
              ", ".join(f"{k} {v:6.2f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if SCORE:
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    N_OPT, L_OPT = 4, 16

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    V = model.llm.lm_head.weight.shape[0]
    for B in [int(a) for a in _args] or [1, 8]:
        inp = synthetic_inputs(cfg, B, PROMPT, modalities=("images", "audios"), seed=2, device=dev)
        g = torch.Generator().manual_seed(4)
        conts = [[torch.randint(3, V, (L_OPT,), generator=g).tolist() for _ in range(N_OPT)] for _ in range(B)]
        with torch.no_grad():
            emb, t_prep = timed(lambda: model.prepare_inputs_for_generation(inp)[0])
            _, t_prep = timed(lambda: model.prepare_inputs_for_generation(inp)[0])
            rep = emb.repeat_interleave(N_OPT, 0)
            arms = {"score": lambda: model.llm.score(inputs_embeds=emb, continuations=conts),
                    "recompute": lambda: model.llm.score(inputs_embeds=emb, continuations=conts, use_cache=False)}
            a, b = arms["score"](), arms["recompute"]()          # warm-up, and the two paths agree to bf16 noise
            print(f"B={B:2d} n={N_OPT} len={L_OPT} prompt rows {emb.shape[1]}: largest |score - recompute| over the token "
                  f"log-probabilities {float((a.token_logprobs - b.token_logprobs).abs().max()):.3f}, over the sums "
                  f"{float((a.sums - b.sums).abs().max()):.3f}; same argmax option for "
                  f"{int((a.sums.argmax(1) == b.sums.argmax(1)).sum())} of {B} prompts", flush=True)
            model.llm.generate(inputs_embeds=rep, max_new_tokens=8, eos_token_id=-1)
            ms = {k: [] for k in ("score", "recompute", "steps")}
            for r in range(REPS):
                for k in ms:
                    if k == "steps":
                        t = {new: timed(lambda: model.llm.generate(inputs_embeds=rep, max_new_tokens=new, eos_token_id=-1))[1]
                             for new in (8, 72)}
                        ms[k].append((t[72] - t[8]) / 64 * L_OPT)
                    else:
                        ms[k].append(timed(arms[k])[1])
                    print(f"B={B:2d} rep {r} {k:9s}: {ms[k][-1]:8.2f} ms", flush=True)
        sp = {k: max(v) - min(v) for k, v in ms.items()}
        print(f"B={B:2d} n={N_OPT} len={L_OPT} prompt rows {emb.shape[1]}: score {med(ms['score']):8.2f} ms (spread {sp['score']:.2f}), "
              f"recompute {med(ms['recompute']):8.2f} ms (spread {sp['recompute']:.2f}), {L_OPT} teacher-forced steps at "
              f"{B * N_OPT} rows {med(ms['steps']):8.2f} ms (spread {sp['steps']:.2f}); recompute / score = "
              f"{med(ms['recompute']) / med(ms['score']):.2f}, steps / score = {med(ms['steps']) / med(ms['score']):.2f}; towers + "
              f"alignment once per prompt {t_prep:.2f} ms (outside every arm)", flush=True)
    sys.exit(0)
if GRAMMAR:
    import random
    from macaw_llm_amd import ops
    from macaw_llm_amd.grammar import TokenDFA
    V = model.llm.lm_head.weight.shape[0]
    JSON = r'\{"name": "[a-z ]{1,12}", "n": (0|[1-9]\d?)\}'
    rnd = random.Random(7)
    vocab = [None] * 3 + [bytes([i]) for i in range(256)]
    vocab += [bytes(rnd.choice(b'{}":, name0123456789abcxyz.-') for _ in range(rnd.randint(2, 17))) for _ in range(V - len(vocab))]
    free = TokenDFA.from_edges(1, [(0, t, 0) for t in range(V)], [0], vocab_size=V)
    json_g = TokenDFA.from_regex(JSON, vocab)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731

    def timed(fn, n=1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) / n

    # the making of a table: the byte walk on the device and the trim, first call (kernel load) and a fresh object after it
    for name, make in (("35-state JSON", lambda: TokenDFA.from_regex(JSON, vocab)),
                       ("[a-z ]{1,3000}", lambda: TokenDFA.from_regex("[a-z ]{1,3000}", vocab))):
        t0 = time.perf_counter(); g = make(); host = time.perf_counter() - t0
        times = []
        for _ in range(3):
            g = make()
            (tab, _s), t = timed(lambda: g.table(dev))
            times.append(t * 1e3)
        cn = torch.from_numpy(g.char_next).to(dev)
        tb, to = torch.from_numpy(g._tok_bytes.copy()).to(dev), torch.from_numpy(g._tok_off).to(dev)
        _, tk = timed(lambda: ops.grammar_build(cn, tb, to), 5)
        print(f"table {name}: {g.n_states} states x {V} tokens = {g.n_states * V * 4 / 2 ** 20:.1f} MiB; host compile "
              f"{host * 1e3:.1f} ms; TokenDFA.table (upload + mk_grammar_build + trim + flags) {times[0]:.1f} ms the first time, "
              f"{med(times[1:]):.1f} ms after; the mk_grammar_build launch with its allocation alone {tk * 1e3:.2f} ms", flush=True)
        del tab, g
    ARMS = {"greedy": None, "free": free, "json": json_g}
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms, msW = {a: [] for a in ("greedy", "free")}, {a: [] for a in ("greedy", "json")}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            gen = lambda arm, new: model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, pad_token_id=0, grammar=ARMS[arm])  # noqa: E731
            rows = gen("json", 72)
            W = rows.shape[1]
            LO = 8 if W > 16 else 3                 # the shorter call, whose prefill and first steps the difference cancels
            texts = [b"".join(vocab[t] for t in (r[:r.index(0)] if 0 in r else r)) for r in rows.tolist()]
            print(f"B={B:2d}: the json arm ends by itself after W = {W} tokens; row 0 says {texts[0]!r}", flush=True)
            assert torch.equal(gen("free", 72), gen("greedy", 72)), "the free grammar changed the ids"
            # free against greedy over 72 tokens, as the other -ab arms; json against greedy over the json arm's own width
            for rep in range(REPS):
                for arm in ARMS:
                    for book, lo, hi in ((ms, 8, 72), (msW, LO, W)):
                        if arm not in book:
                            continue
                        t = {}
                        for new in (lo, hi):
                            ids, t[new] = timed(lambda: gen(arm, new))
                            assert ids.shape[1] == new, f"{arm} stopped at {ids.shape[1]} of {new} tokens"
                        book[arm].append((t[hi] - t[lo]) / (hi - lo) * 1e3)
                        print(f"B={B:2d} rep {rep} {arm:6s}: decode {book[arm][-1]:6.3f} ms/token over {hi - lo} tokens", flush=True)
        for arm, book in (("free", ms), ("json", msW)):
            spread = max(book["greedy"]) - min(book["greedy"])
            d = med(book[arm]) - med(book["greedy"])
            print(f"B={B:2d}: greedy {med(book['greedy']):6.3f} ms/token, {arm} {med(book[arm]):6.3f} ms/token, {arm} - greedy = "
                  f"{d * 1e3:+7.1f} us per token ({d / med(book['greedy']) * 100:+5.2f} %), greedy run-to-run spread "
                  f"{spread * 1e3:6.1f} us: {'inside' if abs(d) <= spread else 'OUTSIDE'} the spread", flush=True)
        # one launch by itself: 40 launches captured in a hipGraph (no host between them), replayed 4 times between two events
        x = torch.randn(B, V, device=dev).mul_(3).to(torch.bfloat16)
        tab_j, _ = json_g.table(dev)
        tab_f, _ = free.table(dev)
        out = torch.randint(3, V, (B, 256), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
        tok, done = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.bool, device=dev)
        out_e = torch.zeros((B, 256), dtype=torch.long, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        n_dev = torch.tensor([100], dtype=torch.int32, device=dev)
        s_j = (torch.arange(B, dtype=torch.int32, device=dev) * 5) % json_g.n_states
        s_f, end = torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), -1, dtype=torch.int32, device=dev)
        small = ops.SeqTable([[13, V + i] for i in range(3)] + [[V + 9]], dev)      # the neighbours: sequences that never fire
        us = {}
        for name, fn in (("decode_emit", lambda: ops.decode_emit(x, V, 0, -1, tok, done, out_e, st)),
                         ("grammar_mask json", lambda: ops.grammar_mask(x, V, tab_j, s_j, done, -1)),
                         ("grammar_mask free", lambda: ops.grammar_mask(x, V, tab_f, s_f, done, -1)),
                         ("grammar_advance free", lambda: ops.grammar_advance(out, tab_f, s_f, done, end, n_dev)),
                         ("seq_ban 4 seqs", lambda: ops.seq_ban(x, V, out, small, n_dev)),
                         ("stop_match 4 seqs", lambda: ops.stop_match(out, small, done, n_dev))):
            for i in range(5):
                fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(40):
                    fn()
            graph.replay()
            st.zero_()                              # (the emit's output column: 5 + 5 * 40 launches stay inside out_e's 256)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(4):
                graph.replay()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 160 * 1e3
            st.zero_()
            del graph
        assert not bool(done.any()) and s_f.tolist() == [0] * B
        print(f"B={B:2d}: one launch on [B, {V}] bf16 logits, 40 in a hipGraph (device time incl. the gap between two graph nodes): " +
              ", ".join(f"{k} {v:6.2f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if ADAPTERS:
    from macaw_llm_amd import lora
    llm = model.llm
    targets = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    lora.get_peft_model(llm, lora.LoraConfig(r=16, lora_alpha=32, target_modules=targets))
    with torch.no_grad():
        for n, q in llm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn_like(q.float()) * 0.02)
    live = llm._lora
    bank = lora.AdapterBank(llm)
    sd0 = lora.lora_state_dict(llm)
    bank.add("a0", state_dict=sd0, config=live.config)
    for i in (1, 2, 3):                             # three more adapters of the same form with other weights
        g = torch.Generator(device=dev).manual_seed(10 + i)
        sd = {k: (torch.randn(v.shape, generator=g, device=dev) * (0.02 if ".lora_B." in k else 0.01)).to(v.dtype) for k, v in sd0.items()}
        bank.add(f"a{i}", state_dict=sd, config=live.config)
    bank.stacks()                                   # built once, outside the timed calls
    ARMS = ("base", "merged", "names x1", "names x4")

    def call(arm, emb, new):
        B = emb.shape[0]
        # the live adapter is what "merged" measures; the other arms run on the stored weights, so it is set aside for them
        llm._lora = live if arm == "merged" else None
        try:
            names = None if arm in ("base", "merged") else [f"a{b % 4}" if arm == "names x4" else "a0" for b in range(B)]
            return llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, adapter_names=names)
        finally:
            llm._lora = live
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, PROMPT, modalities=("images", "audios"), seed=2, device=dev)
        ms, ttft = {a: [] for a in ARMS}, {a: [] for a in ARMS}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            S0 = emb.shape[1]
            for arm in ARMS:                        # untimed: each arm's first call at this size
                assert call(arm, emb, 4).shape == (B, 4)
            agree = int((call("merged", emb, 8) == call("names x1", emb, 8)).sum())
            print(f"B={B:2d} S0={S0}: merged and names x1 (the same adapter) agree in {agree} of {B * 8} of their first 8 ids "
                  "(one rounding of W + s B A against two roundings of the 16-bit adapter)", flush=True)
            for rep in range(REPS):
                for arm in ARMS:
                    t = {}
                    for new in (1, 8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        ids = call(arm, emb, new)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                        assert ids.shape == (B, new)
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    ttft[arm].append(t[1] * 1e3)
                    print(f"B={B:2d} S0={S0} rep {rep} {arm:9s}: decode {ms[arm][-1]:7.3f} ms/token, first token {ttft[arm][-1]:8.2f} ms", flush=True)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        spr = lambda v: max(v) - min(v)  # noqa: E731
        for a in ARMS:
            print(f"B={B:2d} S0={S0}: {a:9s} {med(ms[a]):7.3f} ms/token (run-to-run spread {spr(ms[a]) * 1e3:6.1f} us = "
                  f"{spr(ms[a]) / med(ms[a]) * 100:4.1f} %), first token {med(ttft[a]):8.2f} ms (spread {spr(ttft[a]):6.2f} ms)", flush=True)
        for a in ("names x1", "names x4"):
            d = med(ms[a]) - med(ms["merged"])
            print(f"B={B:2d} S0={S0}: {a} - merged = {d * 1e3:+8.1f} us per token ({d / med(ms['merged']) * 100:+6.2f} %, "
                  f"{d * 1e3 / (8 * llm.config.num_hidden_layers):5.2f} us per extra launch): "
                  f"{'inside' if abs(d) <= max(spr(ms[a]), spr(ms['merged'])) else 'OUTSIDE'} the larger of the two spreads; "
                  f"first token {med(ttft[a]) - med(ttft['merged']):+8.2f} ms", flush=True)
    sys.exit(0)
if SESSION:
    from macaw_llm_amd import ops
    E = model.llm.model.embed_tokens.weight
    V = model.llm.lm_head.weight.shape[0]
    ARMS = ("session", "fresh")
    for B in [int(a) for a in _args] or [1, 8]:
        inp = synthetic_inputs(cfg, B, PROMPT, modalities=("images", "audios"), seed=2, device=dev)
        ids2 = torch.randint(3, V, (B, 32), generator=torch.Generator().manual_seed(3)).to(dev)
        first, ms, tower = {a: [] for a in ARMS}, {a: [] for a in ARMS}, []
        with torch.no_grad():
            for rep in range(REPS + 1):             # what a follow-up turn through MM_LLMs also skips (rep 0 untimed)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                emb1 = model.prepare_inputs_for_generation(inp)[0]
                torch.cuda.synchronize(); tower.append((time.perf_counter() - t0) * 1e3)
            S0 = emb1.shape[1]
            emb2 = ops.embedding_fwd(E, ids2.reshape(-1)).view(B, 32, -1)

            def turn1():                            # rows for both turns: no regrowth inside the timed call
                return model.llm.generate(inputs_embeds=emb1, max_new_tokens=64, eos_token_id=-1, return_session=True,
                                          session_capacity=S0 + 64 + 33 + 72)
            out1 = turn1()[0]
            cat = torch.cat([emb1, ops.embedding_fwd(E, out1.reshape(-1)).view(B, 64, -1), emb2], dim=1).contiguous()

            def call(arm, new):                     # -> (ids, seconds)
                s = turn1()[1] if arm == "session" else None
                torch.cuda.synchronize(); t0 = time.perf_counter()
                if arm == "session":
                    ids = model.llm.generate(session=s, inputs_embeds=emb2, max_new_tokens=new, eos_token_id=-1)
                else:
                    ids = model.llm.generate(inputs_embeds=cat, max_new_tokens=new, eos_token_id=-1)
                torch.cuda.synchronize()
                return ids, time.perf_counter() - t0
            for arm in ARMS:                                # untimed: each arm's first calls at this size
                call(arm, 1)
            same = [call(arm, 8)[0] for arm in ARMS]
            print(f"B={B:2d} S0={S0}: the arms' first 8 ids agree in {int((same[0] == same[1]).sum())} of {same[0].numel()} places "
                  "(equal up to the last bits of their arithmetic: other GEMM row counts, another attention form)", flush=True)
            for rep in range(REPS):
                for arm in ARMS:
                    t = {}
                    for new in (1, 8, 72):
                        ids, t[new] = call(arm, new)
                        assert ids.shape == (B, new)
                    first[arm].append(t[1] * 1e3)
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} S0={S0} rep {rep} {arm:8s}: first token of turn 2 {first[arm][-1]:8.2f} ms, decode {ms[arm][-1]:6.3f} ms/token",
                          flush=True)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        spr = lambda v: max(v) - min(v)  # noqa: E731
        for a in ARMS:
            print(f"B={B:2d} S0={S0}: {a:8s} first token of turn 2 {med(first[a]):8.2f} ms (run-to-run spread {spr(first[a]):6.2f} ms), "
                  f"{med(ms[a]):6.3f} ms/token (spread {spr(ms[a]) * 1e3:6.1f} us = {spr(ms[a]) / med(ms[a]) * 100:4.1f} %)", flush=True)
        d = med(ms["session"]) - med(ms["fresh"])
        print(f"B={B:2d} S0={S0}: session / fresh = {med(first['session']) / med(first['fresh']):5.3f} to the first token of turn 2 "
              f"({med(first['fresh']) - med(first['session']):+8.2f} ms saved), session - fresh = {d * 1e3:+7.1f} us per token "
              f"({d / med(ms['fresh']) * 100:+5.2f} %): {'inside' if abs(d) <= max(spr(ms['session']), spr(ms['fresh'])) else 'OUTSIDE'} "
              f"the larger of the two spreads; towers + alignment of the first turn, skipped by a follow-up turn through MM_LLMs: "
              f"{med(tower[1:]):8.2f} ms (spread {spr(tower[1:]):6.2f} ms)", flush=True)
        # the variable-length launch of turn 2's prefill by itself: 200 back-to-back launches between two events, after 20
        # warm-up launches, at the continued call's shape (33 new rows per sample over S0 + 64 + 32 keys)
        lcfg = model.llm.config
        H, D = lcfg.num_attention_heads, lcfg.hidden_size
        hd, Lq, Lk, cap = D // H, 33, S0 + 64 + 32, S0 + 64 + 33 + 72
        g = torch.Generator(device=dev).manual_seed(4)
        q = torch.randn((B * Lq, 3 * D), generator=g, device=dev).to(torch.bfloat16)
        kv = torch.randn((B, cap, 2 * D), generator=g, device=dev).to(torch.bfloat16)
        o = torch.empty((B * Lq, D), dtype=torch.bfloat16, device=dev)
        ql = torch.full((B,), Lq, dtype=torch.int32, device=dev)
        kl = torch.full((B,), Lk, dtype=torch.int32, device=dev)
        fn = lambda: ops.flash_attn_varlen_fwd(q, kv, kv, o, ql, kl, B, H, Lq, Lk, hd, 3 * D, Lq * 3 * D, 2 * D, cap * 2 * D,  # noqa: E731
                                               2 * D, cap * 2 * D, D, Lq * D, hd ** -0.5, v_off=D)
        for i in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(200):
            fn()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 200 * 1e3
        print(f"B={B:2d}: one mk_flash_attn_varlen_fwd launch at H={H}, {Lq} query rows over {Lk} keys, hd={hd} (back to back, incl. launch "
              f"gaps): {us:7.1f} us; x {lcfg.num_hidden_layers} layers = {us * lcfg.num_hidden_layers / 1e3:6.2f} ms of the "
              f"{med(first['session']):6.2f} ms to the first token of turn 2", flush=True)
    sys.exit(0)
if NSAMPLE:
    lcfg = model.llm.config
    NL, D = lcfg.num_hidden_layers, lcfg.hidden_size
    SKW = dict(do_sample=True, top_k=50, top_p=0.9, seed=1, eos_token_id=-1)
    ARMS = ("repeat", "shared R=1", "shared R=4")
    for B, n in ((1, 4), (2, 16), (8, 4)):
        inp = synthetic_inputs(cfg, B, PROMPT, modalities=("images", "audios"), seed=2, device=dev)
        ms, ttft, peak = {a: [] for a in ARMS}, {a: [] for a in ARMS}, {}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            S0 = emb.shape[1]
            emb_r = emb.repeat_interleave(n, 0)

            def call(arm, new):
                if arm == "repeat":
                    return model.llm.generate(inputs_embeds=emb_r, max_new_tokens=new, **SKW)
                os.environ["MK_SHARED_ATTN_ROWS"] = arm[-1]
                try:
                    return model.llm.generate(inputs_embeds=emb, max_new_tokens=new, num_samples=n, **SKW)
                finally:
                    del os.environ["MK_SHARED_ATTN_ROWS"]
            # the KV cache of the 72-token call, all layers: [keys | values] rows of 2 D 16-bit elements
            kvb = {"repeat": NL * B * n * (S0 + 72) * 2 * D * 2, "shared R=1": NL * (B * S0 + B * n * 72) * 2 * D * 2}
            kvb["shared R=4"] = kvb["shared R=1"]
            for arm in ARMS:                        # untimed: each arm's first call at this size
                assert call(arm, 4).shape == (B * n, 4)
            for rep in range(REPS):
                for arm in ARMS:
                    t = {}
                    for new in (1, 8, 72):
                        torch.cuda.synchronize(); base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
                        t0 = time.perf_counter()
                        ids = call(arm, new)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                        assert ids.shape == (B * n, new)
                    peak[arm] = torch.cuda.max_memory_allocated() - base
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    ttft[arm].append(t[1] * 1e3)
                    print(f"B={B:2d} n={n:2d} S0={S0} rep {rep} {arm:10s}: decode {ms[arm][-1]:6.3f} ms/token, first token {ttft[arm][-1]:8.2f} ms", flush=True)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        medt = {a: sorted(v)[len(v) // 2] for a, v in ttft.items()}
        spr = {a: max(v) - min(v) for a, v in ms.items()}
        for a in ARMS:
            print(f"B={B:2d} n={n:2d} S0={S0}: {a:10s} {med[a]:6.3f} ms/token (run-to-run spread {spr[a] * 1e3:6.1f} us = {spr[a] / med[a] * 100:4.1f} %), "
                  f"first token {medt[a]:8.2f} ms, KV cache {kvb[a] / 1e9:7.3f} GB allocated (allocator peak over the call {peak[a] / 1e9:7.3f} GB)", flush=True)
        d1 = med["shared R=4"] - med["shared R=1"]
        print(f"B={B:2d} n={n:2d} S0={S0}: shared R=1 / repeat = {med['shared R=1'] / med['repeat']:5.3f} per token, {medt['shared R=1'] / medt['repeat']:5.3f} to the "
              f"first token, KV {kvb['shared R=1'] / kvb['repeat']:5.3f}; tiled - untiled = {d1 * 1e3:+7.1f} us ({d1 / med['shared R=1'] * 100:+5.2f} %): "
              f"{'inside' if abs(d1) <= max(spr['shared R=4'], spr['shared R=1']) else 'OUTSIDE'} the larger of their spreads", flush=True)
    sys.exit(0)
if STOP:
    from macaw_llm_amd import ops
    V = model.llm.lm_head.weight.shape[0]
    # the last id of every sequence lies above the vocabulary: no emitted tail ever equals one, no column is ever banned
    SKW = dict(stop_sequences=[[13, 29871, V + i] for i in range(3)] + [[V + 7]],
               bad_words_ids=[[13, V + i] for i in range(3)] + [[V + 9]])
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {"greedy": [], "stop+ban": []}
        call72 = {"greedy": [], "stop+ban": [], "all stop at 71": []}       # the whole 72-token call, ms
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for mode in ms:                         # untimed: each mode's first call at this batch size
                model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=-1, **(SKW if mode != "greedy" else {}))
            # every sample stops at column 71: each row's own last 16 ids, unless some row's ids end with a sequence earlier
            rows = model.llm.generate(inputs_embeds=emb, max_new_tokens=72, eos_token_id=-1).tolist()
            last = [r[56:] for r in rows]
            early = any(r[c - 15:c + 1] == q for r in rows for q in last for c in range(15, 71))
            LKW = None if early else dict(stop_sequences=last, bad_words_ids=SKW["bad_words_ids"])
            if LKW is not None:
                model.llm.generate(inputs_embeds=emb, max_new_tokens=72, eos_token_id=-1, **LKW)
            for rep in range(REPS):
                for mode in ("greedy", "stop+ban"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        ids = model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, **(SKW if mode != "greedy" else {}))
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                        assert ids.shape[1] == new, f"stopped early at {ids.shape[1]} of {new} tokens: the timing would be of another loop"
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    call72[mode].append(t[72] * 1e3)
                    print(f"B={B:2d} rep {rep} {mode:8s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
                if LKW is not None:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    ids = model.llm.generate(inputs_embeds=emb, max_new_tokens=72, eos_token_id=-1, **LKW)
                    torch.cuda.synchronize(); call72["all stop at 71"].append((time.perf_counter() - t0) * 1e3)
                    assert ids.tolist() == rows, "the samples did not all stop at the last column"
        m72 = {k: sorted(v)[len(v) // 2] for k, v in call72.items() if v}
        print(f"B={B:2d}: the 72-token call, prefill included: " + ", ".join(f"{k} {v:8.3f} ms" for k, v in m72.items()) +
              (f"; all stop at 71 - stop+ban = {(m72['all stop at 71'] - m72['stop+ban']) * 1e3:+7.1f} us per call (the width search: "
               f"72 stop_match launches and two host reads), stop+ban spread {(max(call72['stop+ban']) - min(call72['stop+ban'])) * 1e3:6.1f} us"
               if "all stop at 71" in m72 else "; all stop at 71: not measured (a row's ids repeat)"), flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = max(ms["greedy"]) - min(ms["greedy"])
        diff = med["stop+ban"] - med["greedy"]
        print(f"B={B:2d}: greedy {med['greedy']:6.3f} ms/token, stop+ban {med['stop+ban']:6.3f} ms/token, stop+ban - greedy = "
              f"{diff * 1e3:+7.1f} us ({diff / med['greedy'] * 100:+5.2f} %), greedy run-to-run spread {spread * 1e3:6.1f} us "
              f"({spread / med['greedy'] * 100:4.1f} %): {'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread", flush=True)
        # one launch by itself: 200 back-to-back launches between two events, after 20 warm-up launches
        x = torch.randn(B, V, device=dev).mul_(3).to(torch.bfloat16)
        g = torch.Generator(device=dev).manual_seed(3)
        out = torch.randint(0, V, (B, 256), generator=g, device=dev)
        tok, done = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.bool, device=dev)
        out_e = torch.zeros((B, 256), dtype=torch.long, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        n_dev = torch.tensor([100], dtype=torch.int32, device=dev)
        small = ops.SeqTable(SKW["bad_words_ids"], dev)
        big = ops.SeqTable([[int(c) for c in torch.randint(0, V, (3,), generator=g, device=dev)] + [V + 1] for _ in range(1000)], dev)
        us = {}
        for name, fn in (("decode_emit", lambda: ops.decode_emit(x, V, 0, -1, tok, done, out_e, st)),
                         ("seq_ban 4 seqs", lambda: ops.seq_ban(x, V, out, small, n_dev)),
                         ("seq_ban 1000 seqs", lambda: ops.seq_ban(x, V, out, big, n_dev)),
                         ("stop_match 4 seqs", lambda: ops.stop_match(out, small, done, n_dev)),
                         ("stop_match 1000 seqs", lambda: ops.stop_match(out, big, done, n_dev))):
            for i in range(20):
                fn()
            st.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
            st.zero_()
        assert not bool(done.any())
        print(f"B={B:2d}: one launch on [B, {V}] bf16 logits / 100 generated ids (back to back, incl. launch gaps): " +
              ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if CFG:
    from macaw_llm_amd import ops
    for B in [int(a) for a in _args] or [1, 8, 16]:
        big = synthetic_inputs(cfg, 2 * B, 128, modalities=("images", "audios"), seed=2, device=dev)
        with torch.no_grad():
            emb2 = model.prepare_inputs_for_generation(big)[0]
            emb1 = emb2[:B].contiguous()
            tids = big["input_ids"][:B].long()
            neg = ops.embedding_fwd(model.llm.model.embed_tokens.weight, tids.reshape(-1)).view(B, tids.shape[1], -1)
            call = {"greedy B": lambda n: model.llm.generate(inputs_embeds=emb1, max_new_tokens=n, eos_token_id=-1),
                    "greedy 2B": lambda n: model.llm.generate(inputs_embeds=emb2, max_new_tokens=n, eos_token_id=-1),
                    "guided B": lambda n: model.llm.generate(inputs_embeds=emb1, negative_inputs_embeds=neg, guidance_scale=1.5,
                                                             max_new_tokens=n, eos_token_id=-1)}
            ms = {a: [] for a in call}
            for arm in call:                        # untimed: each arm's first call at this size
                call[arm](4)
            for rep in range(REPS):
                for arm in call:
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        out = call[arm](new)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                        assert out.shape == (2 * B if arm == "greedy 2B" else B, new)
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {arm:9s}: decode {ms[arm][-1]:6.3f} ms/token", flush=True)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        sp = {a: max(v) - min(v) for a, v in ms.items()}
        print(f"B={B:2d}: prompt {emb1.shape[1]} rows, negative prompt {neg.shape[1]} rows; greedy at batch {B} {med['greedy B']:6.3f} "
              f"ms/token (spread {sp['greedy B'] * 1e3:6.1f} us), greedy at batch {2 * B} {med['greedy 2B']:6.3f} ms/token (spread "
              f"{sp['greedy 2B'] * 1e3:6.1f} us), guidance_scale=1.5 at batch {B} {med['guided B']:6.3f} ms/token (spread "
              f"{sp['guided B'] * 1e3:6.1f} us)", flush=True)
        for base in ("greedy 2B", "greedy B"):
            diff = med["guided B"] - med[base]
            print(f"B={B:2d}: guided - {base} = {diff * 1e3:+8.1f} us ({diff / med[base] * 100:+6.2f} %): "
                  f"{'inside' if abs(diff) <= sp[base] else 'OUTSIDE'} the {base} spread", flush=True)
        # one launch by itself: 200 back-to-back launches between two events, after 20 warm-up launches.  The combine runs at
        # scale 1 (the op launches whatever the scale; row b then holds its own log-softmax, which a repeat leaves in place)
        x = torch.randn(2 * B, 32000, device=dev).mul_(3).to(torch.bfloat16)
        ids = ops.argmax_rows(x[:B])
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        st1 = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=dev)      # the step form writes column state[1] - 1 = 0
        book = ops.LogprobState(B, 256, 0, 0, dev)
        feed = torch.empty((2 * B, emb1.shape[2]), dtype=emb1.dtype, device=dev)
        fns = [("cfg_combine", lambda: ops.cfg_combine(x, 32000, B, 1.0)),
               ("decode_emit_logprobs n=0", lambda: ops.decode_emit_logprobs(x[:B], 32000, ids, done, st1, book)),
               ("embedding gather of B tokens", lambda: ops.embedding_fwd(model.llm.model.embed_tokens.weight, ids, out=feed[B:]))]
        us = {}
        for name, fn in fns:
            for i in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
        print(f"B={B:2d}: one launch (back to back, incl. launch gaps), [2B, 32000] bf16 logits: " +
              ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if LOGPROBS:
    from macaw_llm_amd import ops
    ARMS = {"greedy": {}, "logprobs": dict(return_logprobs=True), "top5": dict(return_logprobs=True, top_logprobs=5)}
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {a: [] for a in ARMS}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for kw in ARMS.values():                # untimed: each arm's first call at this batch size
                model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=-1, **kw)
            for rep in range(REPS):
                for arm, kw in ARMS.items():
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        out = model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, **kw)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                        assert (out if arm == "greedy" else out.ids).shape[1] == new
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {arm:8s}: decode {ms[arm][-1]:6.3f} ms/token", flush=True)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        spread = max(ms["greedy"]) - min(ms["greedy"])
        for arm in ("logprobs", "top5"):
            diff = med[arm] - med["greedy"]
            print(f"B={B:2d}: greedy {med['greedy']:6.3f} ms/token, {arm} {med[arm]:6.3f} ms/token, {arm} - greedy = {diff * 1e3:+7.1f} us "
                  f"({diff / med['greedy'] * 100:+5.2f} %), greedy run-to-run spread {spread * 1e3:6.1f} us "
                  f"({spread / med['greedy'] * 100:4.1f} %): {'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread", flush=True)
        # one launch by itself: 200 back-to-back launches between two events, after 20 warm-up launches
        x = torch.randn(B, 32000, device=dev).mul_(3).to(torch.bfloat16)
        ids = ops.argmax_rows(x)
        tok, done = ids.clone(), torch.zeros(B, dtype=torch.bool, device=dev)
        out_e = torch.zeros((B, 256), dtype=torch.long, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        st1 = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=dev)      # the step form writes column state[1] - 1 = 0
        books = {n: ops.LogprobState(B, 256, n, 0, dev) for n in (0, 5, 20)}
        fns = [("argmax_rows", lambda: ops.argmax_rows(x)), ("decode_emit", lambda: ops.decode_emit(x, 32000, 0, -1, tok, done, out_e, st))]
        for n in (0, 5, 20):
            fns.append((f"token_logprobs n={n}", lambda n=n: ops.token_logprobs(x, 32000, ids, n)))
        for n in (0, 5, 20):
            fns.append((f"decode_emit_logprobs n={n}", lambda n=n: ops.decode_emit_logprobs(x, 32000, ids, done, st1, books[n])))
        us = {}
        for name, fn in fns:
            for i in range(20):
                fn()
            st.zero_(); done.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
            st.zero_(); done.zero_()
        print(f"B={B:2d}: one launch on [B, 32000] bf16 logits (back to back, incl. launch gaps): " +
              ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if LOOKUP:
    G = 7
    inp = synthetic_inputs(cfg, 1, 128, modalities=("images", "audios"), seed=2, device=dev)
    with torch.no_grad():
        emb = model.prepare_inputs_for_generation(inp)[0]
        y = model.llm.generate(inputs_embeds=emb, max_new_tokens=72, eos_token_id=-1)
        print(f"greedy output: {len(set(y[0].tolist()))} distinct ids among {y.shape[1]}", flush=True)
        arms = {"greedy": {}, "cold": dict(prompt_lookup_num_tokens=G), "accepting": dict(prompt_lookup_num_tokens=G, input_ids=y)}
        ms, tps = {a: [] for a in arms}, {a: [] for a in arms}
        for kw in arms.values():                    # untimed: each arm's first call
            model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=-1, **kw)
        for rep in range(REPS):
            for arm, kw in arms.items():
                t, st = {}, {}
                for new in (8, 72):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    out = model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, return_lookup_stats=arm != "greedy", **kw)
                    torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ids, st[new] = (out[0], int(out[1][0])) if arm != "greedy" else (out, new)
                    assert ids.shape[1] == new
                ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                tps[arm].append(64 / max(st[72] - st[8], 1))
                print(f"B= 1 rep {rep} {arm:9s}: {ms[arm][-1]:6.3f} ms per emitted token, {tps[arm][-1]:5.2f} tokens per step "
                      f"({st[72]} steps for 72 tokens)", flush=True)
    med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
    for arm in arms:
        sp = max(ms[arm]) - min(ms[arm])
        print(f"B= 1 G={G}: {arm:9s} {med[arm]:6.3f} ms per emitted token ({arm} / greedy = {med[arm] / med['greedy']:5.3f}), "
              f"{sorted(tps[arm])[len(tps[arm]) // 2]:5.2f} tokens per step, ms per step {med[arm] * sorted(tps[arm])[len(tps[arm]) // 2]:6.3f}, "
              f"run-to-run spread {sp * 1e3:6.1f} us ({sp / med[arm] * 100:4.1f} %)", flush=True)
    sys.exit(0)
if BEAM:
    from macaw_llm_amd import ops
    for B, K in ((1, 4), (8, 4), (2, 16)):
        big = synthetic_inputs(cfg, B * K, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {"greedy": [], "beam": []}
        with torch.no_grad():
            emb_g = model.prepare_inputs_for_generation(big)[0]
            emb_b = emb_g[::K].contiguous()         # the beam call's B prompts are B of the greedy call's B * K
            call = {"greedy": lambda n: model.llm.generate(inputs_embeds=emb_g, max_new_tokens=n, eos_token_id=-1),
                    "beam": lambda n: model.llm.generate(inputs_embeds=emb_b, max_new_tokens=n, eos_token_id=-1, num_beams=K)}
            for mode in call:                       # untimed: each mode's first call at this size
                call[mode](4)
            for rep in range(REPS):
                for mode in ("greedy", "beam"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        call[mode](new)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} K={K:2d} rep {rep} {mode:6s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = max(ms["greedy"]) - min(ms["greedy"])
        diff = med["beam"] - med["greedy"]
        print(f"B={B:2d} K={K:2d}: greedy at batch {B * K} {med['greedy']:6.3f} ms/token, num_beams={K} at batch {B} {med['beam']:6.3f} ms/token, "
              f"beam - greedy = {diff * 1e3:+7.1f} us ({diff / med['greedy'] * 100:+5.2f} %), greedy run-to-run spread {spread * 1e3:6.1f} us "
              f"({spread / med['greedy'] * 100:4.1f} %), beam spread {(max(ms['beam']) - min(ms['beam'])) * 1e3:6.1f} us: "
              f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} the greedy spread", flush=True)
        # one selection launch by itself: 200 back-to-back launches between two events, after 20 warm-up launches
        x = torch.randn(B * K, 32000, device=dev).mul_(3).to(torch.bfloat16)
        tok, done = torch.zeros(B * K, dtype=torch.long, device=dev), torch.zeros(B * K, dtype=torch.bool, device=dev)
        out = torch.zeros((B * K, 256), dtype=torch.long, device=dev)
        bs = ops.BeamState(B, K, 256, 0, dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        us = {}
        for name, fn in (("decode_emit", lambda: ops.decode_emit(x, 32000, 0, -1, tok, done, out, st)),
                         ("beam_emit", lambda: ops.beam_emit(x, 32000, K, 0, -1, 1.0, False, bs, st))):
            for i in range(20):
                fn()
            st.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
            st.zero_()
        print(f"B={B:2d} K={K:2d}: one launch on [{B * K}, 32000] bf16 logits (back to back, incl. launch gaps; beam_emit at output "
              f"columns 0 ... 199): " + ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if PROC:
    from macaw_llm_amd import ops
    PKW = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8)
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {"greedy": [], "processors": []}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for mode in ms:                         # untimed: each mode's first call at this batch size
                model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=2, **(PKW if mode == "processors" else {}))
            for rep in range(REPS):
                for mode in ("greedy", "processors"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        ids = model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=2,      # (an eos: min_new_tokens is live)
                                                 **(PKW if mode == "processors" else {}))
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                        assert ids.shape[1] == new, f"stopped early at {ids.shape[1]} of {new} tokens: the timing would be of another loop"
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {mode:10s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = max(ms["greedy"]) - min(ms["greedy"])
        diff = med["processors"] - med["greedy"]
        print(f"B={B:2d}: greedy {med['greedy']:6.3f} ms/token, processors {med['processors']:6.3f} ms/token, processors - greedy = "
              f"{diff * 1e3:+7.1f} us ({diff / med['greedy'] * 100:+5.2f} %), greedy run-to-run spread {spread * 1e3:6.1f} us "
              f"({spread / med['greedy'] * 100:4.1f} %): {'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread", flush=True)
        # one launch by itself: 200 back-to-back launches between two events, after 20 warm-up launches
        x = torch.randn(B, 32000, device=dev).mul_(3).to(torch.bfloat16)
        g = torch.Generator(device=dev).manual_seed(3)
        prompt = torch.randint(0, 32000, (B, 200), generator=g, device=dev)
        p_len = torch.full((B,), 200, dtype=torch.int32, device=dev)
        out = torch.randint(0, 32000, (B, 256), generator=g, device=dev)
        tok, done = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.bool, device=dev)
        out_e = torch.zeros((B, 256), dtype=torch.long, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        n_dev = torch.tensor([100], dtype=torch.int32, device=dev)
        us = {}
        for name, fn in (("decode_emit", lambda: ops.decode_emit(x, 32000, 0, -1, tok, done, out_e, st)),
                         ("logits_process (1.2, 3, 8), 300 ids", lambda: ops.logits_process(x, 32000, out, n_dev, 0, prompt, p_len, 1.2, 3, 8, 2)),
                         ("logits_process (1.2, 0, 0), 300 ids", lambda: ops.logits_process(x, 32000, out, n_dev, 0, prompt, p_len, 1.2, 0, 0, 2)),
                         ("logits_process (1.0, 3, 0), 300 ids", lambda: ops.logits_process(x, 32000, out, n_dev, 0, prompt, p_len, 1.0, 3, 0, 2))):
            for i in range(20):
                fn()
            st.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn()
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
            st.zero_()
        print(f"B={B:2d}: one launch on [B, 32000] bf16 logits (back to back, incl. launch gaps): " +
              ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if WARPERS:
    from macaw_llm_amd import ops
    SKW = dict(do_sample=True, top_k=50, top_p=0.9, seed=1)
    ARMS = {"greedy": {}, "sampled": SKW, "min_p": dict(SKW, min_p=0.05),
            "typ+eps+eta": dict(SKW, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)}
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {a: [] for a in ARMS}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for arm, kw in ARMS.items():        # untimed: each arm's first call (code objects, allocator pools at this size)
                model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=-1, **kw)
            for rep in range(REPS):
                for arm, kw in ARMS.items():
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, **kw)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[arm].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {arm:11s}: decode {ms[arm][-1]:6.3f} ms/token", flush=True)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        spread = {a: max(v) - min(v) for a, v in ms.items()}
        print(f"B={B:2d}: " + ", ".join(f"{a} {med[a]:6.3f} ms/token (spread {spread[a] * 1e3:5.1f} us)" for a in ARMS), flush=True)
        for a in ("min_p", "typ+eps+eta"):
            d = med[a] - med["sampled"]
            print(f"B={B:2d}: {a} - sampled = {d * 1e3:+7.1f} us / token ({d / med['sampled'] * 100:+5.2f} %): "
                  f"{'inside' if abs(d) <= spread['sampled'] else 'OUTSIDE'} the sampled arm's spread", flush=True)
        # the selection launch of each arm by itself: 200 back-to-back launches between two events, after 20 warm-up launches
        x = torch.randn(B, 32000, device=dev).mul_(3).to(torch.bfloat16)
        us = {}
        for name, fn in (("argmax_rows", lambda i: ops.argmax_rows(x)),
                         ("sampled", lambda i: ops.sample_rows(x, None, 1.0, 50, 0.9, 1, i)),
                         ("min_p", lambda i: ops.sample_rows_warp(x, None, 1.0, 50, 0.9, 1, 0.05, step=i)),
                         ("typ+eps+eta", lambda i: ops.sample_rows_warp(x, None, 1.0, 50, 0.9, 1, 0.0, 0.9, 3e-4, 2e-3, step=i)),
                         ("typical k=0 p=1", lambda i: ops.sample_rows_warp(x, None, 1.0, 0, 1.0, 1, 0.0, 0.9, step=i)),
                         ("keep mask typ+eps+eta", lambda i: ops.sample_keep_rows(x, None, 1.0, 50, 0.9, 0.0, 0.9, 3e-4, 2e-3))):
            for i in range(20):
                fn(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn(i)
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
        print(f"B={B:2d}: one launch on [B, 32000] bf16 logits (back to back, incl. launch gaps): " +
              ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if SAMPLE:
    from macaw_llm_amd import ops
    SKW = dict(do_sample=True, top_k=50, top_p=0.9, seed=1)
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {"greedy": [], "sample": []}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for rep in range(REPS):
                for mode in ("greedy", "sample"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, **(SKW if mode == "sample" else {}))
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {mode:6s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = max(ms["greedy"]) - min(ms["greedy"])
        diff = med["sample"] - med["greedy"]
        print(f"B={B:2d}: greedy {med['greedy']:6.3f} ms/token, sampled {med['sample']:6.3f} ms/token, sampled - greedy = {diff * 1e3:+7.1f} us "
              f"({diff / med['greedy'] * 100:+5.2f} %), greedy run-to-run spread {spread * 1e3:6.1f} us ({spread / med['greedy'] * 100:4.1f} %): "
              f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread", flush=True)
        # one selection launch by itself: 200 back-to-back launches between two events, after 20 warm-up launches
        x = torch.randn(B, 32000, device=dev).mul_(3).to(torch.bfloat16)
        us = {}
        for name, fn in (("argmax_rows", lambda i: ops.argmax_rows(x)),
                         ("sample_rows k=50 p=0.9", lambda i: ops.sample_rows(x, None, 1.0, 50, 0.9, 1, i)),
                         ("sample_rows k=0 p=1", lambda i: ops.sample_rows(x, None, 1.0, 0, 1.0, 1, i))):
            for i in range(20):
                fn(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                fn(i)
            e1.record(); torch.cuda.synchronize()
            us[name] = e0.elapsed_time(e1) / 200 * 1e3
        print(f"B={B:2d}: one launch on [B, 32000] bf16 logits (back to back, incl. launch gaps): " +
              ", ".join(f"{k} {v:6.1f} us" for k, v in us.items()), flush=True)
    sys.exit(0)
if RAGGED:
    lcfg = model.llm.config
    NL, D = lcfg.num_hidden_layers, lcfg.hidden_size
    for B in [int(a) for a in _args] or [32]:
        inp = synthetic_inputs(cfg, B, PROMPT, modalities=("images", "audios"), seed=2, device=dev)
        ms = {"mask": [], "none": []}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            S0 = emb.shape[1]
            pads = [round((PROMPT - SHORT) * b / max(B - 1, 1)) for b in range(B)]      # sample b: pads[b] masked rows on the left
            mask = torch.ones((B, S0), dtype=torch.long, device=dev)
            for b, n in enumerate(pads):
                mask[b, :n] = 0
            real = [S0 - n for n in pads]
            kvb = {"mask": NL * sum(n + 40 for n in real) * 2 * D * 2, "none": NL * B * (S0 + 40) * 2 * D * 2}
            for mode in ("none", "mask"):       # untimed: each mode's first call (kernel attributes, allocator pools at this size)
                model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=-1, attention_mask=mask if mode == "mask" else None)
            for rep in range(REPS):
                for mode in ("none", "mask"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1,
                                           attention_mask=mask if mode == "mask" else None)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} S0={S0} real {real[0]} ... {real[-1]} rep {rep} {mode:4s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = (max(ms["none"]) - min(ms["none"])) / med["none"]
        print(f"B={B:2d} S0={S0}, real lengths {real[0]} ... {real[-1]} (sum {sum(real)} of {B * S0}): no mask {med['none']:6.3f} ms/token "
              f"({kvb['none'] / 1e9:6.3f} GB of KV per token), attention_mask {med['mask']:6.3f} ms/token ({kvb['mask'] / 1e9:6.3f} GB), "
              f"mask / none = {med['mask'] / med['none']:5.3f} (no-mask run-to-run spread {spread * 100:4.1f} %)", flush=True)
    sys.exit(0)
if KV8:
    lcfg = model.llm.config
    NL, D, H = lcfg.num_hidden_layers, lcfg.hidden_size, lcfg.num_attention_heads
    for B in [int(a) for a in _args] or [1, 8, 32]:
        inp = synthetic_inputs(cfg, B, PROMPT, modalities=("images", "audios"), seed=2, device=dev)
        ms = {None: [], "fp8": []}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            S0 = emb.shape[1]
            ctx = S0 + 40                           # keys a step reads at the middle of the timed window (tokens 8 ... 72)
            kvb = {None: NL * B * ctx * 2 * D * 2, "fp8": NL * B * ctx * (2 * D + 2 * H * 4)}
            for rep in range(REPS):
                for mode in (None, "fp8"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, kv_cache=mode)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} S0={S0} rep {rep} kv {mode or 'bf16':4s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = (max(ms[None]) - min(ms[None])) / med[None]
        print(f"B={B:2d} S0={S0}: kv bf16 {med[None]:6.3f} ms/token ({kvb[None] / 1e9:6.3f} GB of KV per token), kv fp8 "
              f"{med['fp8']:6.3f} ms/token ({kvb['fp8'] / 1e9:6.3f} GB), fp8 / bf16 = {med['fp8'] / med[None]:5.3f} "
              f"(bf16 run-to-run spread {spread * 100:4.1f} %)", flush=True)
    sys.exit(0)
if MX4:
    proj = [lyr.fused_weights() + (lyr.self_attn.o_proj.weight, lyr.mlp.down_proj.weight) for lyr in model.llm.model.layers]
    proj = [w for ws in proj for w in ws]
    head = model.llm.lm_head.weight
    MODES = (None, "fp8", "mxfp4")
    BYTES = {None: sum(2 * w.numel() for w in proj + [head]), "fp8": sum(w.numel() + 4 * w.shape[0] for w in proj + [head]),
             "mxfp4": sum(w.numel() // 2 + w.numel() // 32 for w in proj) + head.numel() + 4 * head.shape[0]}
    print("streamed per token: " + ", ".join(f"{m or 'bf16'} {BYTES[m] / 1e9:.3f} GB" for m in MODES) +
          " (mxfp4: e2m1 codes + E8M0 exponents of the layers' projections, e4m3 lm_head)", flush=True)
    with torch.no_grad():       # the quantised copies are made here, outside the timed calls
        for mode in MODES[1:]:
            model.llm.generate(inputs_embeds=model.prepare_inputs_for_generation(_w)[0], max_new_tokens=4, eos_token_id=-1,
                               decode_weights=mode)
    for B in [int(a) for a in _args] or [1, 8, 16, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {m: [] for m in MODES}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for mode in MODES:  # untimed: each mode's first call at this batch size (kernel attributes, allocator pools)
                model.llm.generate(inputs_embeds=emb, max_new_tokens=4, eos_token_id=-1, decode_weights=mode)
            for rep in range(REPS):
                for mode in MODES:
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, decode_weights=mode)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {mode or 'bf16':5s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = {m: (max(v) - min(v)) / med[m] for m, v in ms.items()}
        print(f"B={B:2d}: " + ", ".join(f"{m or 'bf16'} {med[m]:6.3f} ms/token ({BYTES[m] / med[m] / 1e9:4.2f} TB/s, spread "
                                        f"{spread[m] * 100:4.1f} %)" for m in MODES) +
              f"; fp8 / bf16 = {med['fp8'] / med[None]:5.3f}, mxfp4 / bf16 = {med['mxfp4'] / med[None]:5.3f}, "
              f"mxfp4 / fp8 = {med['mxfp4'] / med['fp8']:5.3f}: mxfp4 is "
              f"{'OUTSIDE' if med['fp8'] - med['mxfp4'] > max(spread['fp8'] * med['fp8'], spread['mxfp4'] * med['mxfp4']) else 'inside'}"
              " the fp8 / mxfp4 spreads", flush=True)
    sys.exit(0)
if AB:
    streamed = [lyr.fused_weights() + (lyr.self_attn.o_proj.weight, lyr.mlp.down_proj.weight) for lyr in model.llm.model.layers]
    streamed = [w for ws in streamed for w in ws] + [model.llm.lm_head.weight]
    BYTES = {None: sum(2 * w.numel() for w in streamed), "fp8": sum(w.numel() + 4 * w.shape[0] for w in streamed)}
    print(f"streamed per token: bf16 {BYTES[None] / 1e9:.3f} GB, fp8 {BYTES['fp8'] / 1e9:.3f} GB (e4m3 bytes + f32 scales)")
    with torch.no_grad():       # the e4m3 copies are made here, outside the timed calls
        model.llm.generate(inputs_embeds=model.prepare_inputs_for_generation(_w)[0], max_new_tokens=4, eos_token_id=-1,
                           decode_weights="fp8")
    for B in [int(a) for a in _args] or [1, 8, 16, 32]:
        inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
        ms = {None: [], "fp8": []}
        with torch.no_grad():
            emb = model.prepare_inputs_for_generation(inp)[0]
            for rep in range(REPS):
                for mode in (None, "fp8"):
                    t = {}
                    for new in (8, 72):
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1, decode_weights=mode)
                        torch.cuda.synchronize(); t[new] = time.perf_counter() - t0
                    ms[mode].append((t[72] - t[8]) / 64 * 1e3)
                    print(f"B={B:2d} rep {rep} {mode or 'bf16':4s}: decode {ms[mode][-1]:6.3f} ms/token", flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = (max(ms[None]) - min(ms[None])) / med[None]
        print(f"B={B:2d}: bf16 {med[None]:6.3f} ms/token ({BYTES[None] / med[None] / 1e9:4.2f} TB/s), fp8 {med['fp8']:6.3f} ms/token "
              f"({BYTES['fp8'] / med['fp8'] / 1e9:4.2f} TB/s), fp8 / bf16 = {med['fp8'] / med[None]:5.3f} "
              f"(bf16 run-to-run spread {spread * 100:4.1f} %)", flush=True)
    sys.exit(0)
BATCHES = [int(a) for a in _args] or [1, 8, 32]
SK = [v for v in os.environ.get("BG_SKINNY32", "").split(",") if v]
for B, sk in [(B, s) for B in BATCHES for s in (SK if (SK and B > 16) else [None])]:
    if sk is not None:
        os.environ["MK_GEMM_SKINNY32"] = sk
    var = None if sk is None else f"skinny32 {sk}"
    inp = synthetic_inputs(cfg, B, 128, modalities=("images", "audios"), seed=2, device=dev)
    with torch.no_grad():
        emb, am, _ = model.prepare_inputs_for_generation(inp)
        for new in (8, 72):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = model.llm.generate(inputs_embeds=emb, max_new_tokens=new, eos_token_id=-1)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if new == 8: t8 = dt
        per_tok = (dt - t8) / 64
        print(("" if var is None else f"[{var}] ") + f"B={B:2d}: prompt S={emb.shape[1]}, prefill+8 tok {t8 * 1e3:7.1f} ms, decode {per_tok * 1e3:6.2f} ms/token "
              f"= {B / per_tok:7.0f} tokens/s (weights streamed once per token: {13.5 / per_tok / 1e3:4.2f} TB/s)")
