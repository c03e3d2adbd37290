"""Shared by tests/test_speculative_cpu.py and tests/test_speculative_gpu.py: hand-written rows for
``spec_advance`` (state before the call and, written out by hand, the state after), a runner that
applies an implementation to them, and the Python simulation of the accept / draft rules on a
finished answer."""
import torch

NGRAM = 2


def case(idx, samp, hist, h0, pos, ctr, new, want, eos=-1, ngram=NGRAM, finished=False, accept=True, lh=None):
    """One row.  ``hist`` lists the corpus as far as it is written (padded with -1 up to ``lh``);
    ``want``: the fields that change, by hand: idx, out (the row's answer columns, -1 = untouched),
    hist (prefix), pos, ctr, nsteps, finished."""
    return dict(idx=idx, samp=samp, hist=hist, h0=h0, pos=pos, ctr=ctr, new=new, eos=eos, ngram=ngram,
                finished=finished, accept=accept, lh=lh or len(hist) + len(idx) + 2, want=want)


# K = 3 (Q = 4) unless noted.  Corpus letters are small ints; position p sits at hist[h0 + p].
CASES = {
    # corpus 5 6 7 5 6 | last emitted 6 at pos 4; drafts 7 5 6 all confirmed, one more token (9)
    "all_accepted": case(idx=[6, 7, 5, 6], samp=[7, 5, 6, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4, ctr=2, new=20,
                         want=dict(out={2: 7, 3: 5, 4: 6, 5: 9}, hist=[5, 6, 7, 5, 6, 7, 5, 6, 9], pos=8, ctr=6,
                                   nsteps=1, finished=False,
                                   # tail (6, 9) never occurred: every draft is the last token
                                   idx=[9, 9, 9, 9])),
    # the first draft is already wrong: one token
    "none_accepted": case(idx=[6, 7, 5, 6], samp=[5, 5, 6, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4, ctr=2, new=20,
                          want=dict(out={2: 5}, hist=[5, 6, 7, 5, 6, 5], pos=5, ctr=3, nsteps=1, finished=False,
                                    # tail (6, 5): latest earlier start 1?  c[1:3] = 6 7 no; none -> last token
                                    idx=[5, 5, 5, 5])),
    # drafts 7 5 6, sampler 7 8 ..: one draft kept, then the sampler's own 8
    "mismatch_in_the_middle": case(idx=[6, 7, 5, 6], samp=[7, 8, 6, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4, ctr=2,
                                   new=20,
                                   want=dict(out={2: 7, 3: 8}, hist=[5, 6, 7, 5, 6, 7, 8], pos=6, ctr=4, nsteps=1,
                                             finished=False, idx=[8, 8, 8, 8])),
    # eos (= 5) is the second accepted token: the row ends there, the third is not emitted
    "eos_among_accepted": case(idx=[6, 7, 5, 6], samp=[7, 5, 6, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4, ctr=2, new=20,
                               eos=5,
                               want=dict(out={2: 7, 3: 5}, hist=[5, 6, 7, 5, 6, 7, 5], pos=6, ctr=4, nsteps=1,
                                         finished=True,
                                         # tail (7, 5) at start 2: continuation 6 7 5 (period 3)
                                         idx=[5, 6, 7, 5])),
    # eos (= 9) only behind the first mismatch: ignored
    "eos_among_rejected": case(idx=[6, 7, 5, 6], samp=[7, 8, 9, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4, ctr=2, new=20,
                               eos=9,
                               want=dict(out={2: 7, 3: 8}, hist=[5, 6, 7, 5, 6, 7, 8], pos=6, ctr=4, nsteps=1,
                                         finished=False, idx=[8, 8, 8, 8])),
    # all three drafts right but the answer has room for two more tokens only
    "answer_full_before_a_plus_1": case(idx=[6, 7, 5, 6], samp=[7, 5, 6, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4,
                                        ctr=2, new=4,
                                        want=dict(out={2: 7, 3: 5}, hist=[5, 6, 7, 5, 6, 7, 5], pos=6, ctr=4,
                                                  nsteps=1, finished=True, idx=[5, 6, 7, 5])),
    # a finished row: nothing changes but the draft (which its discarded steps feed on)
    "finished_row_untouched": case(idx=[6, 1, 1, 1], samp=[7, 5, 6, 9], hist=[5, 6, 7, 5, 6], h0=0, pos=4, ctr=2,
                                   new=20, finished=True,
                                   want=dict(out={}, hist=[5, 6, 7, 5, 6], pos=4, ctr=2, nsteps=0, finished=True,
                                             # tail (5, 6) at start 0: continuation 7 5 6
                                             idx=[6, 7, 5, 6])),
    # draft only (accept=False).  Corpus 3 4 3 4: tail (3, 4) at start 0, period 2 < K = 3: 3 4 3
    "period_shorter_than_k": case(idx=[0, 0, 0, 0], samp=[0, 0, 0, 0], hist=[3, 4, 3, 4], h0=0, pos=3, ctr=1, new=20,
                                  accept=False,
                                  want=dict(out={}, hist=[3, 4, 3, 4], pos=3, ctr=1, nsteps=0, finished=False,
                                            idx=[4, 3, 4, 3])),
    "no_match": case(idx=[0, 0, 0, 0], samp=[0, 0, 0, 0], hist=[1, 2, 3, 4, 5], h0=0, pos=4, ctr=1, new=20,
                     accept=False,
                     want=dict(out={}, hist=[1, 2, 3, 4, 5], pos=4, ctr=1, nsteps=0, finished=False,
                               idx=[5, 5, 5, 5])),
    # n = 2 = ngram: no search
    "n_not_above_ngram": case(idx=[0, 0, 0, 0], samp=[0, 0, 0, 0], hist=[8, 8], h0=0, pos=1, ctr=1, new=20,
                              accept=False,
                              want=dict(out={}, hist=[8, 8], pos=1, ctr=1, nsteps=0, finished=False,
                                        idx=[8, 8, 8, 8])),
    # hint 7 1 2 9 4 (h0 = 5), sequence 6 1 2 at positions 0..2: tail (1, 2) found in the hint at 1
    "match_inside_the_hint": case(idx=[0, 0, 0, 0], samp=[0, 0, 0, 0], hist=[7, 1, 2, 9, 4, 6, 1, 2], h0=5, pos=2,
                                  ctr=1, new=20, accept=False,
                                  want=dict(out={}, hist=[7, 1, 2, 9, 4, 6, 1, 2], pos=2, ctr=1, nsteps=0,
                                            finished=False, idx=[2, 9, 4, 6])),
    # (1, 2) at starts 0 and 4: the later one, continuation 8 1 2
    "latest_match_preferred": case(idx=[0, 0, 0, 0], samp=[0, 0, 0, 0], hist=[1, 2, 3, 9, 1, 2, 8, 1, 2], h0=0,
                                   pos=8, ctr=1, new=20, accept=False,
                                   want=dict(out={}, hist=[1, 2, 3, 9, 1, 2, 8, 1, 2], pos=8, ctr=1, nsteps=0,
                                             finished=False, idx=[2, 8, 1, 2])),
}


def run_rows(fn, rows, device="cpu"):
    """Apply ``fn`` (``ops.spec_advance`` / the oracle) to the rows as ONE batch -> the state
    tensors afterwards (on the CPU).  The rows must share Q, new, eos, ngram and accept."""
    r0 = rows[0]
    assert all((len(r["idx"]), r["new"], r["eos"], r["ngram"], r["accept"]) ==
               (len(r0["idx"]), r0["new"], r0["eos"], r0["ngram"], r0["accept"]) for r in rows)
    lh = max(r["lh"] for r in rows)
    hist = torch.full((len(rows), lh), -1, dtype=torch.int32)
    for b, r in enumerate(rows):
        hist[b, :len(r["hist"])] = torch.tensor(r["hist"], dtype=torch.int32)
    st = dict(idx=torch.tensor([r["idx"] for r in rows], dtype=torch.long),
              samp=torch.tensor([r["samp"] for r in rows], dtype=torch.long), hist=hist,
              h0=torch.tensor([r["h0"] for r in rows], dtype=torch.int32),
              pos=torch.tensor([r["pos"] for r in rows], dtype=torch.int32),
              ctr=torch.tensor([r["ctr"] for r in rows], dtype=torch.int32),
              nsteps=torch.zeros(len(rows), dtype=torch.int32),
              finished=torch.tensor([r["finished"] for r in rows], dtype=torch.bool),
              out=torch.full((len(rows), r0["new"]), -1, dtype=torch.long))
    st = {k: v.to(device) for k, v in st.items()}
    fn(st["idx"], st["samp"], st["hist"], st["h0"], st["pos"], st["ctr"], st["nsteps"], st["finished"], st["out"],
       r0["eos"], r0["ngram"], r0["accept"])
    return {k: v.cpu() for k, v in st.items()}


def check_case(st, b, r):
    """Row b of the state after the call against the hand-written expectation of case r."""
    w = r["want"]
    assert st["idx"][b].tolist() == w["idx"], ("idx", st["idx"][b].tolist())
    out = [-1] * r["new"]
    for c, v in w["out"].items():
        out[c] = v
    assert st["out"][b].tolist() == out, ("out", st["out"][b].tolist())
    hist = w["hist"] + [-1] * (st["hist"].shape[1] - len(w["hist"]))
    assert st["hist"][b].tolist() == hist, ("hist", st["hist"][b].tolist())
    got = (int(st["pos"][b]), int(st["ctr"][b]), int(st["nsteps"][b]), bool(st["finished"][b]))
    assert got == (w["pos"], w["ctr"], w["nsteps"], w["finished"]), got
    assert torch.equal(st["samp"][b], torch.tensor(r["samp"])) and int(st["h0"][b]) == r["h0"]


def draft(corpus, K, ngram=NGRAM):
    """The K prompt-lookup drafts after ``corpus`` (a list of ints)."""
    n = len(corpus)
    best = -1
    for i in range(n - ngram - 1, -1, -1):
        if corpus[i:i + ngram] == corpus[n - ngram:]:
            best = i
            break
    if n <= ngram or best < 0:
        return [corpus[-1]] * K
    per = n - best - ngram
    return [corpus[best + ngram + (j % per)] for j in range(K)]


def simulate(prompt, answer, hint, K, ngram=NGRAM):
    """The verify steps of one row, from its tokens alone: ``answer`` = every token the row drew
    (an eos included, which can only be its last).  -> the drafts accepted in each step, one entry
    per step.  The first token comes from the prefill; a step then emits the leading drafts that
    equal the answer's next tokens and one more, as far as the answer goes."""
    c, accepted = 1, []
    while c < len(answer):
        d = draft(list(hint) + list(prompt) + list(answer[:c]), K, ngram)
        rem = len(answer) - c
        a = 0
        while a < K and a < rem and d[a] == answer[c + a]:
            a += 1
        e = min(a + 1, rem)
        accepted.append(e - 1)
        c += e
    return accepted
