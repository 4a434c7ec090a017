"""Host model of the token-level state machine of gq_sample_topk_fsm / gq_sample_full_fsm (include/gq_hip.h), in numpy: the mask rows
gq_token_fsm_build leaves and the transition the publishing lane makes -- written from the contract over the four CSR arrays, with loops
over states and edges (no searchsorted, no shared code with guidedquant_amd/token_fsm.py) -- and the machines the GPU tests use.

    mask row s  = (default_next[s] < 0 ? all ones : all zeros), then per edge of the row: bit set (edge_next < 0) or cleared,
                  then OR base_suppress, then the bits at and past V in the last word set
    step(s, t)  = edge_next of the edge (s, t) when there is one, else default_next[s]; t outside [0, V) (the token of an empty
                  candidate set) or a result of -1 leaves the state as it is
"""
import numpy as np

EMPTY_TOKEN = 0x7FFFFFFF


def words(V):
    return (V + 31) // 32


def mask_rows(row_ptr, edge_tok, edge_next, default_next, V, base=None):
    """uint32 [S, ceil(V / 32)]: row s is the FORBIDDEN set of state s in the layout of `suppress`"""
    S, W = len(default_next), words(V)
    out = np.zeros((S, W), dtype=np.uint32)
    for s in range(S):
        bits = np.full(W * 32, default_next[s] < 0, dtype=bool)
        for e in range(int(row_ptr[s]), int(row_ptr[s + 1])):
            t = int(edge_tok[e])
            if 0 <= t < V:
                bits[t] = edge_next[e] < 0
        if base is not None:
            bits |= np.unpackbits(np.ascontiguousarray(base, dtype=np.uint32).view(np.uint8), bitorder="little").astype(bool)
        bits[V:] = True
        out[s] = np.packbits(bits, bitorder="little").view(np.uint32)
    return out


def row_allowed(row, V):
    """the ids a mask row allows, ascending"""
    bits = np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")[:V]
    return np.nonzero(bits == 0)[0]


def step(row_ptr, edge_tok, edge_next, default_next, V, s, tok):
    """the state after `tok` was drawn in state s"""
    if not 0 <= tok < V:
        return s
    nx = int(default_next[s])
    for e in range(int(row_ptr[s]), int(row_ptr[s + 1])):
        if int(edge_tok[e]) == tok:
            nx = int(edge_next[e])
            break
    return nx if nx >= 0 else s


def csr(fsm):
    """the four arrays of a TokenFSM, for the functions above"""
    return fsm.row_ptr, fsm.edge_tok, fsm.edge_next, fsm.default_next


# ------------------------------------------------------------------------------------------------ the machines of the GPU tests
def layout_edges(V):
    """the tokens where a wrong word or bit shows: 0, 31, 32, V - 1 (those that exist)"""
    return sorted({t for t in (0, 31, 32, V - 1) if 0 <= t < V})


def builder_machine(S, V, seed=0):
    """(n_states, edges, default_next) for the builder test: the rows cycle through 0, 1, 2 and 33 edges (as many as V holds), at the layout
    tokens first; every third state allows by default and its edges are forbidden exceptions.  Not validated (dead ends are the builder's
    to lay out like any other row)."""
    rng = np.random.default_rng(1000 + seed)
    edges, dn = [], []
    for s in range(S):
        n = min((0, 1, 2, 33)[s % 4], V)
        lay = layout_edges(V)
        toks = lay[:n]
        if n > len(toks):
            rest = np.setdiff1d(np.arange(V), lay)
            toks = toks + rng.choice(rest, size=min(n - len(toks), rest.size), replace=False).tolist()
        default_allows = s % 3 == 2
        dn.append((s + 1) % S if default_allows else -1)
        for j, t in enumerate(sorted(toks)):
            # (a default-allowed state: mostly forbidden exceptions, one edge that allows and leads elsewhere)
            edges.append((s, int(t), -1 if default_allows and j % 4 != 3 else (s + j) % S))
    return S, edges, dn


def chain_machine(tokens):
    """state i allows exactly tokens[i] and leads to i + 1, the last one back to 0"""
    n = len(tokens)
    return n, [(i, int(t), (i + 1) % n) for i, t in enumerate(tokens)], [-1] * n


def to_csr(S, edges, default_next):
    """(row_ptr, edge_tok, edge_next, default_next) as int32 arrays from a list of (state, token, next) -- no validation"""
    edges = sorted(edges)
    row_ptr = np.zeros(S + 1, dtype=np.int32)
    for s, _, _ in edges:
        row_ptr[s + 1] += 1
    return (np.cumsum(row_ptr).astype(np.int32), np.array([e[1] for e in edges], dtype=np.int32), np.array([e[2] for e in edges], dtype=np.int32),
            np.array(default_next, dtype=np.int32))


def ring_machine(V, S=5, seed=0, hot=()):
    """a machine without dead ends whose states alternate between the two kinds: an even state allows a listed set only (the layout tokens,
    some of `hot` -- tokens the logits favour -- and random ones, each leading to some state), an odd one allows everything but a few
    exceptions (half of `hot` among them) and leads to the next state, with some edges that lead elsewhere"""
    rng = np.random.default_rng(7000 + seed)
    hot = [int(t) for t in hot if 0 <= t < V]
    edges, dn = [], []
    for s in range(S):
        if s % 2 == 0:
            n = min(V // 2 + 1, 40)
            toks = set(layout_edges(V)[:n]) | set(hot[s % 3::3]) | set(rng.choice(V, size=n, replace=False).tolist())
            dn.append(-1)
            edges += [(s, int(t), int(rng.integers(S))) for t in sorted(toks)]
        else:
            forb = set(hot[::2]) | set(rng.choice(V, size=min(V // 3, 10), replace=False).tolist())
            away = set(rng.choice(V, size=min(V // 3, 10), replace=False).tolist()) - forb
            dn.append((s + 1) % S)
            edges += [(s, int(t), -1) for t in sorted(forb)] + [(s, int(t), int(rng.integers(S))) for t in sorted(away)]
    return S, edges, dn
