"""Speculative decoding, host side: the prompt-lookup drafter and the
acceptance rule of Engine(speculative=K).

A verify step feeds T = K + 1 tokens per sequence through one forward: the
last emitted token followed by K drafted ones.  Row j's argmax is the token
greedy decode would emit after inputs 0..j, so draft j is right exactly
when it equals argmax j - 1, and every right draft is a token that cost no
weight pass of its own.  Both functions are pure.
"""
from __future__ import annotations

from typing import List, Optional, Sequence


def ngram_draft(ids: Sequence[int], k: int, max_ngram: int = 3) -> List[int]:
    """Prompt lookup: for n = max_ngram down to 1, find the most recent
    earlier occurrence of the last n tokens of `ids` and return the (at
    most k) tokens that followed it; [] when no n matches."""
    ids = list(ids)
    L = len(ids)
    if k <= 0:
        return []
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = ids[L - n:]
        # an earlier occurrence ends before the last token, so at least
        # one token follows it
        for start in range(L - n - 1, -1, -1):
            if ids[start:start + n] == tail:
                return ids[start + n:start + n + k]
    return []


def pad_draft(draft: Sequence[int], k: int, input_id: int) -> List[int]:
    """The K tokens fed after the input token: the draft, padded with its
    last token, or with the input token when it is empty.  Padding is
    wrong guesses; accept() never looks at it."""
    draft = list(draft)[:k]
    fill = draft[-1] if draft else input_id
    return draft + [fill] * (k - len(draft))


def accept(draft: Sequence[int], argmax: Sequence[int],
           stop_id: Optional[int], room: int) -> List[int]:
    """The tokens a verify step emits.  `draft` is the unpadded draft,
    argmax[j] the model's greedy token after the input token and drafts
    0..j-1, `room` (>= 1) how many tokens the request may still take.
    Emits argmax[0..j] while draft[i] == argmax[i] for i < j: the accepted
    drafts plus one, ending early at stop_id or when room is used up,
    exactly where token-by-token decode would end."""
    out: List[int] = []
    for j, tok in enumerate(argmax):
        out.append(tok)
        if len(out) >= room or (stop_id is not None and tok == stop_id):
            break
        if j >= len(draft) or draft[j] != tok:
            break
    return out
