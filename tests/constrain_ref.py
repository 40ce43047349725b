"""Independent restatements for trie-constrained decoding: a dict trie, HF's PrefixConstrainedLogitsProcessor in torch (pinned to
HF's own class by tests/golden/constrain.npz) and the host walk.  Nothing here imports the package under test."""
import torch

EOS = 1


class DictTrie:
    """phrase sets as nested dicts: {token: subtree}; a phrase is closed by EOS (added when missing)"""

    def __init__(self, sets, eos=EOS):
        self.eos = eos
        self.roots = []
        for phrases in sets:
            root = {}
            for p in phrases:
                p = list(p)
                if not p or p[-1] != eos:
                    p = p + [eos]
                node = root
                for t in p:
                    node = node.setdefault(int(t), {})
            self.roots.append(root)

    def node(self, prefix, set=0):
        """the subtree behind prefix, None off the trie"""
        node = self.roots[set]
        for t in prefix:
            if node is None:
                return None
            node = node.get(int(t))
        return node

    def allowed(self, prefix, set=0):
        """the callback's answer: the children, [eos] off the trie and at a leaf"""
        node = self.node(prefix, set)
        return sorted(node) if node else [self.eos]

    def contains(self, seq, set=0):
        seq = list(seq)
        if not seq or seq[-1] != self.eos:
            seq = seq + [self.eos]
        return self.eos not in seq[:-1] and self.node(seq, set) is not None

    def phrases(self, set=0):
        out = []

        def rec(node, pre):
            if not node:
                out.append(pre)
            for t in sorted(node):
                rec(node[t], pre + [t])
        rec(self.roots[set], [])
        return out


def callback(trie, sets, num_beams, skip=1):
    """HF's prefix_allowed_tokens_fn over a DictTrie: image = batch_id (HF passes batch_id = row // num_beams itself), the phrase
    starts behind the first `skip` ids of the row (the start token and a decoder prompt)"""
    def fn(batch_id, sent):
        return trie.allowed(sent.tolist()[skip:], sets[batch_id])
    return fn


def hf_constrain(scores, histories, trie, sets, num_beams, skip=1):
    """PrefixConstrainedLogitsProcessor.__call__ restated: scores [rows, V] f32, histories [rows, L] int64; rows = images * num_beams"""
    mask = torch.full_like(scores, -float("inf"))
    for r in range(scores.shape[0]):
        allowed = trie.allowed(histories[r].tolist()[skip:], sets[r // num_beams])
        mask[r, allowed] = 0
    return scores + mask


def walk(table, prefix, set=0):
    """the node of klab's CSR tables (child_off, child_tok, child_node, roots as lists / arrays) behind prefix, -1 off the trie"""
    off, tok, node, roots = table
    cur = int(roots[set])
    for t in prefix:
        if cur < 0:
            return -1
        nxt = -1
        for e in range(int(off[cur]), int(off[cur + 1])):
            if int(tok[e]) == int(t):
                nxt = int(node[e])
                break
        cur = nxt
    return cur


def random_phrases(rng, n, vocab, max_len=6, lo=2):
    """n distinct phrases (lengths 1 .. max_len over ids >= lo) by random walks that mostly extend an earlier phrase's prefix: shared
    prefixes, and phrases that are prefixes of others"""
    seen, out = set(), []
    while len(out) < n:
        if out and rng.random() < 0.7:
            base = rng.choice(out)
            pre = base[:rng.randint(0, len(base))]
        else:
            pre = []
        length = rng.randint(max(1, len(pre)), max_len)
        p = tuple(pre + [rng.randrange(lo, vocab) for _ in range(length - len(pre))])
        if p and p not in seen:
            seen.add(p)
            out.append(list(p))
    return out
