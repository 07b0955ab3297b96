"""KV cache for the bundled inference engine — contiguous slot-based
cache sized against 288 GB HBM3E per MI355X (no reference counterpart;
SkyPilot delegates serving to user images)."""
from __future__ import annotations

from typing import List

import torch

from skypilot_amd import ops
from skypilot_amd.models.llama import LlamaConfig

KV_DTYPES = ("bf16", "fp8")


class KVCache:
    """One [max_batch, max_seq, Hkv, D] K and V tensor per layer.

    kv_dtype "bf16" (the default) stores the rows as they are.  "fp8"
    stores each row of one (token, kv head) as D e4m3fn codes in `k` / `v`
    (uint8) plus one power-of-two exponent byte in `k_exp` / `v_exp`
    (uint8 [max_batch, max_seq, Hkv]); ops.kv_quantize is the format."""

    def __init__(self, cfg: LlamaConfig, max_batch: int, max_seq: int,
                 device, dtype=torch.bfloat16, kv_dtype: str = "bf16"):
        if kv_dtype not in KV_DTYPES:
            raise ValueError(
                f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        self.cfg = cfg
        self.max_batch = max_batch
        self.max_seq = max_seq
        self.kv_dtype = kv_dtype
        self.k: List[torch.Tensor] = []
        self.v: List[torch.Tensor] = []
        self.k_exp: List[torch.Tensor] = []
        self.v_exp: List[torch.Tensor] = []
        fp8 = kv_dtype == "fp8"
        for _ in range(cfg.num_layers):
            shape = (max_batch, max_seq, cfg.num_kv_heads, cfg.head_dim)
            if fp8:
                dtype = torch.uint8
                # exponent 127 with code 0: a zero row at scale 1
                self.k_exp.append(torch.full(shape[:3], 127, device=device,
                                             dtype=torch.uint8))
                self.v_exp.append(torch.full(shape[:3], 127, device=device,
                                             dtype=torch.uint8))
            self.k.append(torch.zeros(shape, device=device, dtype=dtype))
            self.v.append(torch.zeros(shape, device=device, dtype=dtype))
        # host-side slot lengths (engine keeps the authoritative copy)
        self.lens = [0] * max_batch

    @staticmethod
    def bytes_needed(cfg: LlamaConfig, max_batch: int, max_seq: int,
                     kv_dtype: str = "bf16") -> int:
        if kv_dtype not in KV_DTYPES:
            raise ValueError(
                f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        # per (token, kv head) row: D bf16, or D codes and an exponent byte
        row = (cfg.head_dim + 1 if kv_dtype == "fp8" else cfg.head_dim * 2)
        return (2 * cfg.num_layers * max_batch * max_seq *
                cfg.num_kv_heads * row)

    @classmethod
    def sized_for_memory(cls, cfg: LlamaConfig, max_seq: int,
                         budget_bytes: int, device,
                         cap: int = 256, kv_dtype: str = "bf16") -> "KVCache":
        """Pick max_batch to fill the HBM budget (288 GB minus weights)."""
        per_slot = cls.bytes_needed(cfg, 1, max_seq, kv_dtype)
        max_batch = max(1, min(cap, budget_bytes // per_slot))
        return cls(cfg, max_batch, max_seq, device, kv_dtype=kv_dtype)

    # ---- writes -----------------------------------------------------------
    def write_rows_fp8(self, layer: int, k: torch.Tensor, v: torch.Tensor,
                       slots: torch.Tensor, starts: torch.Tensor,
                       lens: torch.Tensor) -> None:
        """fp8 cache: quantise and store a whole batch, k/v [n, S, Hkv, D]
        and int32 [n] tensors on their device; row i < lens[b] goes to
        [slots[b], starts[b] + i] (ops.kv_write_fp8, one launch)."""
        ops.kv_write_fp8(k, v, self.k[layer], self.v[layer],
                         self.k_exp[layer], self.v_exp[layer], slots,
                         starts, lens)

    def _i32(self, val: int) -> torch.Tensor:
        return torch.tensor([val], dtype=torch.int32,
                            device=self.k[0].device)

    def write_prefill(self, layer: int, slot: int, k: torch.Tensor,
                      v: torch.Tensor, length: int) -> None:
        """k/v: [1, S_padded, Hkv, D]; store the first `length` rows."""
        if self.kv_dtype == "fp8":
            self.write_rows_fp8(layer, k[:1], v[:1], self._i32(slot),
                                self._i32(0), self._i32(length))
            return
        self.k[layer][slot, :length] = k[0, :length]
        self.v[layer][slot, :length] = v[0, :length]

    def write_append(self, layer: int, slot: int, start: int,
                     k: torch.Tensor, v: torch.Tensor, length: int) -> None:
        """k/v: [1, Sq_padded, Hkv, D], one chunk of a longer prompt;
        store its first `length` rows at [slot, start:start+length]."""
        if self.kv_dtype == "fp8":
            self.write_rows_fp8(layer, k[:1], v[:1], self._i32(slot),
                                self._i32(start), self._i32(length))
            return
        self.k[layer][slot, start:start + length] = k[0, :length]
        self.v[layer][slot, start:start + length] = v[0, :length]

    def write_decode(self, layer: int, slots: torch.Tensor,
                     pos: torch.Tensor, k: torch.Tensor,
                     v: torch.Tensor) -> None:
        """k/v: [n, 1, Hkv, D] new tokens; slots/pos: [n] int64.  With an
        fp8 cache this quantises in torch: the CPU and eager fallback (the
        GPU decode step writes from ops.attn_decode_qkv_fp8)."""
        if self.kv_dtype == "fp8":
            self.k[layer][slots, pos], self.k_exp[layer][slots, pos] = \
                ops.kv_quantize(k[:, 0])
            self.v[layer][slots, pos], self.v_exp[layer][slots, pos] = \
                ops.kv_quantize(v[:, 0])
            return
        self.k[layer][slots, pos] = k[:, 0]
        self.v[layer][slots, pos] = v[:, 0]

    def free(self, slot: int) -> None:
        self.lens[slot] = 0
