"""Decoding into a closed set of phrases: a token trie held on the device, walked and applied by the decoding session itself.

    trie = constrain.TokenTrie.from_sequences(class_names_ids, vocab_size=V, eos_token_id=1)   # once per answer set
    trie.to("cuda")
    best = model.generate(images, src, constraint=trie)                       # greedy: the arg-max phrase at every branch
    top5, scores = model.generate(images, src, constraint=trie, num_beams=5, num_return_sequences=5, return_scores=True)

It is HF's `prefix_allowed_tokens_fn` (PrefixConstrainedLogitsProcessor) without the Python callback per row and step: at every
position every row may only choose a child of the trie node it stands on, everything else scores -inf (klab_constrain_rows,
csrc/constrain.hip).  A phrase is an id list in label format (no start token); it is closed by EOS, which is added when missing.
A row that stands on a leaf (its phrase is complete) or off the trie may only choose EOS -- HF itself raises off the trie.

Tables (int32, CSR): child_off [n_nodes + 1], child_tok [n_edges] ascending within a node, child_node
[n_edges], roots [n_sets].  EOS is an ordinary edge to a leaf; a phrase that is a prefix of another has that edge beside the
others.  Several independent phrase sets share one table, one root each (from_sequence_sets; generate's constraint_set names the set
per image).  Nodes are numbered by depth, then in the lexicographic order of the phrases, so the edges are stored in CSR order as
they are found."""
import itertools

import numpy as np
import torch


class TokenTrie:
    def __init__(self, child_off, child_tok, child_node, roots, vocab_size, eos_token_id):
        self._np = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (child_off, child_tok, child_node, roots))
        self.vocab_size, self.eos_token_id = int(vocab_size), int(eos_token_id)
        off, tok, node, roots = self._np
        if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != tok.size or tok.shape != node.shape or roots.size < 1 or \
                (np.diff(off) < 0).any():
            raise ValueError("inconsistent trie tables")
        n = off.size - 1
        if (tok.size and (tok.min() < 0 or tok.max() >= self.vocab_size or node.min() < 0 or node.max() >= n)) or roots.min() < 0 or \
                roots.max() >= n:
            raise ValueError("trie tables hold ids outside the vocabulary or the node range")
        self.child_off, self.child_tok, self.child_node, self.roots = (torch.from_numpy(a) for a in self._np)

    # ---- construction ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_sequences(cls, seqs, vocab_size, eos_token_id=1):
        """seqs: a list of id lists, label format without the start token; a trailing EOS is optional"""
        return cls.from_sequence_sets([seqs], vocab_size, eos_token_id)

    @classmethod
    def from_sequence_sets(cls, sets, vocab_size, eos_token_id=1):
        """several independent phrase sets in one table, set i under roots[i].  Runs on the host in numpy from the sorted phrase
        matrix: one pass per depth, no Python loop per node."""
        V, eos = int(vocab_size), int(eos_token_id)
        if V < 1 or not 0 <= eos < V:
            raise ValueError(f"`eos_token_id` ({eos_token_id}) is outside the vocabulary of {vocab_size}")
        sets = [list(s) for s in sets]
        if not sets or any(len(s) == 0 for s in sets):
            raise ValueError("every phrase set needs at least one phrase")
        seqs = [p for s in sets for p in s]
        n = len(seqs)
        which = np.repeat(np.arange(len(sets), dtype=np.int64), np.fromiter((len(s) for s in sets), np.int64, len(sets)))
        lens = np.fromiter((len(p) for p in seqs), np.int64, n)
        flat = np.fromiter(itertools.chain.from_iterable(seqs), np.int64, int(lens.sum()))
        if flat.size and (flat.min() < 0 or flat.max() >= V):
            raise ValueError(f"a phrase holds ids outside [0, {V})")
        width = int(lens.max()) + 1
        # column 0 = the set, columns 1 .. len the tokens, then EOS when the phrase does not bring its own, then -1
        mat = np.full((n, width + 1), -1, np.int64)
        mat[:, 0] = which
        start = np.cumsum(lens) - lens
        mat[np.repeat(np.arange(n), lens), 1 + np.arange(flat.size) - np.repeat(start, lens)] = flat
        rows = np.arange(n)
        closed = (lens > 0) & (mat[rows, lens] == eos)
        if ((mat[:, 1:] == eos).sum(1) != closed).any():
            raise ValueError("a phrase holds EOS inside; EOS closes a phrase")
        mat[rows[~closed], lens[~closed] + 1] = eos
        lens = lens + ~closed  # tokens with the closing EOS
        # sorted and merged: no row is a prefix of another (each ends with its only EOS)
        order = np.lexsort(mat.T[::-1])
        mat, lens = mat[order], lens[order]
        keep = np.ones(n, bool)
        keep[1:] = (mat[1:] != mat[:-1]).any(1)
        mat, lens = mat[keep], lens[keep]
        n = mat.shape[0]
        # lcp[i]: columns row i shares with row i - 1.  The node of (row i, depth d) -- the prefix of d tokens -- is new iff d >= lcp[i]
        differ = np.ones((n, width + 1), bool)
        differ[1:] = mat[1:] != mat[:-1]
        lcp = differ.argmax(1)  # (rows differ somewhere)
        depth = np.arange(width + 1)
        new = (depth[None, :] >= lcp[:, None]) & (depth[None, :] <= lens[:, None])
        per_depth = new.sum(0)
        base = np.cumsum(per_depth) - per_depth
        # ids by depth, then row; a row that shares the node takes the id of the row that opened it
        ids = np.cumsum(new, 0) - 1 + base[None, :]
        roots = ids[np.nonzero(new[:, 0])[0], 0]
        d_idx, r_idx = np.nonzero(new.T[1:])  # depth-major, rows ascending: parents ascending, tokens ascending within a parent
        d_idx = d_idx + 1
        parent, tok, node = ids[r_idx, d_idx - 1], mat[r_idx, d_idx], ids[r_idx, d_idx]
        n_nodes = int(per_depth.sum())
        if n_nodes >= 2 ** 31 - 1:
            raise ValueError("the trie has more than 2^31 nodes")
        off = np.zeros(n_nodes + 1, np.int64)
        np.cumsum(np.bincount(parent, minlength=n_nodes), out=off[1:])
        return cls(off, tok, node, roots, V, eos)

    # ---- storage -----------------------------------------------------------------------------------------------------------
    @property
    def n_nodes(self):
        return self._np[0].size - 1

    @property
    def n_edges(self):
        return self._np[1].size

    @property
    def n_sets(self):
        return self._np[3].size

    @property
    def device(self):
        return self.child_off.device

    def to(self, device):
        """moves the tables (the host copy the queries below read stays); returns self, as CiderD.to"""
        self.child_off, self.child_tok, self.child_node, self.roots = (
            t.to(device).contiguous() for t in (self.child_off, self.child_tok, self.child_node, self.roots))
        return self

    def state_dict(self):
        off, tok, node, roots = (torch.from_numpy(a.copy()) for a in self._np)
        return dict(child_off=off, child_tok=tok, child_node=node, roots=roots, vocab_size=self.vocab_size,
                    eos_token_id=self.eos_token_id)

    @classmethod
    def from_state_dict(cls, sd):
        return cls(*(torch.as_tensor(sd[k]).cpu().numpy() for k in ("child_off", "child_tok", "child_node", "roots")),
                   sd["vocab_size"], sd["eos_token_id"])

    # ---- host queries (the device kernel's rules) --------------------------------------------------------------------------------
    def child(self, node, tok):
        """the node behind edge `tok` of `node`; -1 off the trie"""
        off, ctok, cnode, _ = self._np
        if node < 0:
            return -1
        lo, hi = int(off[node]), int(off[node + 1])
        i = lo + int(np.searchsorted(ctok[lo:hi], tok))
        return int(cnode[i]) if i < hi and ctok[i] == tok else -1

    def walk(self, prefix, set=0):
        """the node reached from the set's root over `prefix`; -1 off the trie"""
        if not 0 <= int(set) < self.n_sets:
            raise ValueError(f"`set` ({set}) is outside the {self.n_sets} sets of the trie")
        node = int(self._np[3][int(set)])
        for t in prefix:
            node = self.child(node, int(t))
        return node

    def allowed(self, prefix, set=0):
        """the ids a row with this history may choose, ascending; [eos] at a leaf and off the trie"""
        node = self.walk(prefix, set)
        off, ctok = self._np[0], self._np[1]
        if node < 0 or off[node] == off[node + 1]:
            return [self.eos_token_id]
        return ctok[off[node]:off[node + 1]].tolist()

    def contains(self, seq, set=0):
        """whether `seq` (a trailing EOS optional) is a phrase of the set"""
        seq = [int(t) for t in seq]
        if not seq or seq[-1] != self.eos_token_id:
            seq = seq + [self.eos_token_id]
        if self.eos_token_id in seq[:-1]:
            return False
        return self.walk(seq, set) >= 0
