"""Guarded buffers for tests of the C ABI's memory contract (include/vcg.h: the caller passes every buffer and a workspace
of exactly the queried size; outputs are overwritten).

An arena is ONE uint8 tensor laid out as [guard | payload | guard].  Each guard is 64 KiB: a multiple of 256 B, so the payload
keeps the 256-byte alignment of a torch allocation (the float4 / 16-byte paths of the kernels assume it), and wide enough that
a stray access of up to a tile lands in memory the test owns -- nothing here is meant to fault.

  input arena      payload = the tensor, guards = 0xFF: every fp32 word and every bf16 half-word of a guard is a NaN, so an
                   out-of-range element that reaches any output shows there as a NaN
  output arena     payload prefilled with 0xFF ("overwritten": no NaN may survive where a value is written), guards = a fixed
                   byte pattern
  workspace arena  payload = exactly the queried byte count (not rounded up, no slack), prefilled with a byte the test chooses

``check()`` (after the call and a stream synchronise) asserts that both guards still hold their pattern bit for bit.
"""
import torch

GUARD = 64 * 1024
NAN_BYTE = 0xFF
JUNK_BYTE = 0x3F          # 0x3F3F3F3F = 0.747 (fp32), 0x3F3F = 0.746 (bf16): finite junk


def _pattern():
    i = torch.arange(GUARD, dtype=torch.int64)
    return ((i * 37 + 11) % 251).to(torch.uint8)          # position dependent: a shifted copy of the guard does not match


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, nbytes, device, payload_fill=NAN_BYTE, nan_guards=False, name="arena"):
        self.nbytes, self.device, self.name = int(nbytes), device, name
        self.buf = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device=device)
        self.pattern = torch.full((GUARD,), NAN_BYTE, dtype=torch.uint8) if nan_guards else _pattern()
        self.pattern = self.pattern.to(device)
        self.buf[:GUARD] = self.pattern
        self.buf[GUARD + self.nbytes:] = self.pattern
        if payload_fill is not None and self.nbytes:
            self.payload.fill_(payload_fill)

    @property
    def payload(self):
        return self.buf[GUARD:GUARD + self.nbytes]

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def guard(self, side):
        return self.buf[:GUARD] if side == "front" else self.buf[GUARD + self.nbytes:]

    def view(self, dtype, shape=None):
        t = self.payload.view(dtype)
        return t if shape is None else t.view(*shape)

    def untouched(self, byte=NAN_BYTE):
        """does the payload still hold its prefill"""
        return bool((self.payload == byte).all().item()) if self.nbytes else True

    def check(self):
        if self.buf.is_cuda:
            torch.cuda.current_stream().synchronize()
        for side in ("front", "back"):
            bad = (self.guard(side) != self.pattern).nonzero().flatten()
            if bad.numel():
                first, last = int(bad[0].item()), int(bad[-1].item())
                if side == "front":       # offsets relative to the payload's first byte (negative: before it)
                    first, last = first - GUARD, last - GUARD
                else:                     # ... and to the byte behind its last
                    first, last = self.nbytes + first, self.nbytes + last
                raise GuardError("%s: %s guard overwritten: %d byte(s), payload-relative offsets %d .. %d (payload %d bytes)"
                                 % (self.name, side, bad.numel(), first, last, self.nbytes))


def input_arena(t, device, name="input"):
    """the payload holds tensor t (any dtype, made contiguous); guards read as NaN in fp32 and in bf16"""
    t = t.contiguous()
    raw = t.view(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8)
    a = Arena(raw.numel(), device, payload_fill=None, nan_guards=True, name=name)
    a.payload.copy_(raw)
    a.dtype, a.shape = t.dtype, tuple(t.shape)
    return a


def output_arena(shape, dtype, device, name="output"):
    n = 1
    for s in shape:
        n *= int(s)
    a = Arena(n * torch.empty(0, dtype=dtype).element_size(), device, payload_fill=NAN_BYTE, name=name)
    a.dtype, a.shape = dtype, tuple(int(s) for s in shape)
    return a


def workspace_arena(nbytes, device, fill=NAN_BYTE, name="workspace"):
    return Arena(nbytes, device, payload_fill=fill, name=name)
