"""The schedule of ``train/generate.py::generate_continuous`` as a pure-Python oracle, and the
prompt / budget sets its CPU and GPU tests share."""

LENS = [1, 5, 24, 9, 3, 17, 12, 30, 7]            # nine prompts ...
BUDGETS = [12, 3, 8, 1, 12, 5, 10, 2, 6]           # ... and budgets that all differ: slots turn over without an eos
NEW = 12


def simulate(answer_lens, budgets, slots, every, has_eos):
    """The schedule written down in ``generate_continuous``'s docstring, without a model.

    ``answer_lens[i]``: the number of tokens prompt i draws up to and including its first eos (None,
    or anything above its budget: it never draws one).  ``budgets[i]``: its n.  Returns
    ``{"replays", "prefills", "slot": [...], "steps": [...]}`` -- ``slot[i]`` None and ``steps[i]`` 0
    for a prompt with budget 0.  One round: admit (the lowest free slot takes the next waiting
    prompt, one prefill per round with an admission), run ``min(every, min(n - d))`` replays, look
    (only with an eos: a flag is up once d >= the answer length), retire ``d == n`` or flagged."""
    P = len(budgets)
    waiting = [i for i in range(P) if budgets[i] > 0]
    slot, steps = [None] * P, [0] * P
    occ = {}
    replays = prefills = 0
    while occ or waiting:
        free = [s for s in range(slots) if s not in occ]
        admitted = False
        while free and waiting:
            s, i = free.pop(0), waiting.pop(0)
            occ[s], slot[i], admitted = [i, 1], s, True
        prefills += admitted
        run = min(every, min(budgets[i] - d for i, d in occ.values()))
        replays += run
        for v in occ.values():
            v[1] += run
        for s in sorted(occ):
            i, d = occ[s]
            flagged = has_eos and answer_lens[i] is not None and d >= answer_lens[i]
            if d == budgets[i] or flagged:
                steps[i] = d - 1
                del occ[s]
    return {"replays": replays, "prefills": prefills, "slot": slot, "steps": steps}


def static_replays(budgets, slots):
    """Decode steps of the static arm: consecutive groups of ``slots`` prompts, each group running
    until its largest budget is drawn (the first token comes from the prefill)."""
    return sum(max(budgets[g:g + slots]) - 1 for g in range(0, len(budgets), slots))


def stats_match(stats, sim):
    return all(stats[k] == sim[k] for k in ("replays", "prefills", "slot", "steps"))
