"""CPU restatement of `find-pairs`.  Per candidate (A = template = target, B = complement = query) the
specification itself: a one-contig index of A alone (tests/_map_oracle.py, imported as it is) and B mapped against it;
then the acceptance rule and the one-pair-per-read rule in plain Python, written from the issue's text and not from
poreover_amd/pairs.py."""
import _map_oracle as O


def map_candidate(names, seqs, a, b, cache=None):
    """the Hit (or None) of read b against an index that holds read a alone"""
    if cache is None:
        cache = {}
    if a not in cache:
        cache[a] = O.Index([names[a]], [seqs[a]])
    return O.map_read(cache[a], seqs[b])


def map_candidates(names, seqs, candidates):
    cache = {}
    return [map_candidate(names, seqs, a, b, cache) for a, b in candidates]


def decide(names, seqs, candidates, hits, min_identity=0.6, min_cover=0.5):
    """-> (pairs as (A, B) index tuples ordered by template name, one dict per candidate)"""
    recs = []
    for (a, b), h in zip(candidates, hits):
        r = {"template": names[a], "complement": names[b], "mapped": h is not None, "accepted": False, "paired": False}
        if h is not None:
            r["identity"] = h.mlen / h.blen
            r["cover"] = max((h.q_en - h.q_st) / len(seqs[b]), (h.r_en - h.r_st) / len(seqs[a]))
            r["accepted"] = h.strand == -1 and r["identity"] >= min_identity and r["cover"] >= min_cover
            for f in ("strand", "q_st", "q_en", "r_st", "r_en", "mlen", "blen", "NM"):
                r[f] = getattr(h, f)
        recs.append(r)
    ranked = sorted([i for i, r in enumerate(recs) if r["accepted"]],
                    key=lambda i: (-recs[i]["mlen"], names[candidates[i][0]], names[candidates[i][1]]))
    used, pairs = set(), []
    for i in ranked:
        a, b = candidates[i]
        if a in used or b in used:
            continue
        used |= {a, b}
        recs[i]["paired"] = True
        pairs.append((a, b))
    return sorted(pairs, key=lambda p: names[p[0]]), recs


def find_pairs(names, seqs, candidates, min_identity=0.6, min_cover=0.5):
    return decide(names, seqs, candidates, map_candidates(names, seqs, candidates), min_identity, min_cover)
