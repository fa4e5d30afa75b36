"""Event representations on the device: the producers of the event tensors the backbone consumes.

Mirror of the reference ``StackedHistogram`` (data/utils/representations.py:36-117): same constructor arguments, same
``construct(x, y, pol, time) -> uint8 (2*bins, H, W)``, ``get_shape`` / dtype helpers — computed by one HIP scatter
kernel + one clamp/narrow pass (rvt_stacked_histogram, rvt_amd/csrc/events.hpp) instead of ``put_(accumulate=True)``.
Integer work: bit-identical to the reference, including its accumulator wrap-around for hot pixels.

``EventSequenceBuilder`` is the batched producer: B raw event streams in, the whole ``(T, B, 2*bins, H', W')`` uint8 sequence
out (rvt_event_sequence, rvt_amd/csrc/evseq.hpp), with the reference's window slicing (scripts/genx/preprocess_dataset.py:
480-534: ``searchsorted`` side='right' / 'left' in duration mode, ``max(end - N, 0)`` in count mode) and its half-scale
``nearest-exact`` down-sampling of the 1 Mpx sensor done on the device.  Half-scale nearest-exact picks source pixel 2i + 1, so
only events with odd x AND odd y reach the output: the builder drops the other three quarters before the atomic and counts
straight into H/2 x W/2, never forming the full-size image.  Bit-identical to ``construct`` per window + ``interpolate``.

  * ``build(streams, ts_end_us, out=None, bounds_out=None) -> (planes, bounds)``: streams = B tuples ``(x, y, p, t)`` of 1-D
    device tensors (``t`` int64 microseconds; ``x, y, p`` all int16, all int32 or all int64: 14 B per event in the compact form),
    ts_end_us int64 ``[T]`` or ``[B][T]``.  ``out`` may be any contiguous uint8 ``(T, B, C, H', W')`` tensor, e.g. a view into
    the buffer a graphed step reads or the input of ``augment_planes``; bounds int64 ``[B][T][2]`` = (start, end) indices.
  * ``make_table`` / ``write_table`` / ``build_from_table``: the pieces, for callers that keep their buffers.  The table rows
    hold ADDRESSES and the event counts, which the kernels read on the device: capture ``build_from_table`` in a hipGraph,
    then rewrite events and window ends in place, ``write_table`` the new counts (up to the buffers' capacity), and replay.
  * Polarity < 0 counts as 0, as the reference's reader clips it (preprocess_dataset.py:181).

``MixedDensityEventStack`` mirrors the reference's second representation (data/utils/representations.py:130-218): same
constructor, ``construct(x, y, pol, time) -> int8 (bins, H, W)`` (rvt_mixed_density_stack), and
``EventSequenceBuilder(..., representation='mixed_density')`` builds the whole int8 ``(T, B, bins, H', W')`` sequence
(rvt_event_sequence_mixed) with the same table, bounds, workspace and graph-capture contract; half-scale is the reference's
``downsample_ev_repr`` (preprocess_dataset.py:467-477), i.e. the odd pixels again.  Polarity 1 / 0 adds +1 / -1 to bin
``floor(clamp(bins - log(tn) / log(1/2), min=0))`` of its pixel, ``tn`` the fp32 normalised time clamped to [1e-6, 1 - 1e-6];
then the prefix sum over the bins, the int8 wrap and, when ``count_cutoff`` (0..127) is given, the clamp to +-cutoff.
The device takes the bin from the binary exponent of ``tn`` (``bins + floor(log2(tn))``, no logarithm), which is the exact
value of that expression.  Span contract: the output is bit-identical to the reference wherever a window's span
``t[-1] - t[0]`` is at most 2^20 us (every duration-mode configuration the reference ships uses 50 ms).  From 2^22 us upward
the reference's own fp32 ``log`` quotient rounds to an integer for events a few ulps below a power of two and puts them one
bin too high (span 2^24, offset 8 388 606: reference bin 9, exact bin 8); the device returns the mathematically exact bin there.
int8 planes go straight into ``RNNDetector.forward`` / ``forward_sequence`` (no float32 copy).

``t`` must be non-decreasing when the windows are sliced (the searches and the bin rule assume it, as the reference does).
The reference reader's repair (``H5Reader._correct_time``, preprocess_dataset.py:163-172: ``t[i] = max(0, t[0..i])``) is
``repair_time(streams_or_table, carry=None, out_repaired=False)`` here (rvt_event_time_repair, rvt_amd/csrc/evprep.hpp), in place
on the device, and ``EventSequenceBuilder(..., repair_time=True)`` runs it over the table ahead of the bounds launch.  With a
``carry`` tensor (int64 ``[B]``) a stream delivered in chunks gets the repair of the concatenated stream.  Raw Prophesee
recordings come in through ``rvt_amd.recordings``.

Out of scope: reading H5 files.  There is no PyTorch fallback: a missing kernel raises.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L


class StackedHistogram:
    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int] = None, fastmode: bool = True):
        assert bins >= 1 and height >= 1 and width >= 1
        self.bins, self.height, self.width = bins, height, width
        if count_cutoff is None:                              # representations.py:52-57
            self.count_cutoff = 255
        else:
            assert count_cutoff >= 1
            self.count_cutoff = min(count_cutoff, 255)
        self.fastmode = fastmode
        self.channels = 2
        self._scratch = None

    @staticmethod
    def get_numpy_dtype() -> np.dtype:
        return np.dtype('uint8')

    @staticmethod
    def get_torch_dtype() -> torch.dtype:
        return torch.uint8

    @property
    def dtype(self) -> torch.dtype:
        return torch.uint8

    def get_shape(self) -> Tuple[int, int, int]:
        return 2 * self.bins, self.height, self.width

    def construct(self, x: torch.Tensor, y: torch.Tensor, pol: torch.Tensor, time: torch.Tensor) -> torch.Tensor:
        dev = x.device
        assert y.device == pol.device == time.device == dev
        for t in (x, y, pol, time):
            assert not torch.is_floating_point(t) and not torch.is_complex(t)      # representations.py:78-81
        assert x.numel() == y.numel() == pol.numel() == time.numel()
        cells = 2 * self.bins * self.height * self.width
        if self._scratch is None or self._scratch.device != dev:
            self._scratch = torch.empty(cells, dtype=torch.int32, device=dev)
        out = torch.empty(self.get_shape(), dtype=torch.uint8, device=dev)
        x, y, pol, time = (t.to(torch.int64).contiguous() for t in (x, y, pol, time))
        L.call('rvt_stacked_histogram', L.ptr(x), L.ptr(y), L.ptr(pol), L.ptr(time), x.numel(), self.bins, self.height,
               self.width, self.count_cutoff, int(self.fastmode), L.ptr(self._scratch), L.ptr(out), L.stream_of(out))
        return out


class MixedDensityEventStack:
    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int] = None, allow_compilation: bool = False):
        assert bins >= 1 and height >= 1 and width >= 1       # representations.py:133-138
        self.bins, self.height, self.width = bins, height, width
        self.count_cutoff = count_cutoff
        if count_cutoff is not None:                          # representations.py:140-142; None = no clamp
            assert isinstance(count_cutoff, int)
            assert 0 <= count_cutoff <= 2 ** 7 - 1
        self.allow_compilation = allow_compilation            # the reference's torch.compile switch: nothing to compile here
        self._scratch = None

    @staticmethod
    def get_numpy_dtype() -> np.dtype:
        return np.dtype('int8')

    @staticmethod
    def get_torch_dtype() -> torch.dtype:
        return torch.int8

    @property
    def dtype(self) -> torch.dtype:
        return torch.int8

    def get_shape(self) -> Tuple[int, int, int]:
        return self.bins, self.height, self.width

    def construct(self, x: torch.Tensor, y: torch.Tensor, pol: torch.Tensor, time: torch.Tensor) -> torch.Tensor:
        dev = x.device
        assert y.device == pol.device == time.device == dev
        for t in (x, y, pol, time):
            assert not torch.is_floating_point(t) and not torch.is_complex(t)      # representations.py:167-170
        assert x.numel() == y.numel() == pol.numel() == time.numel()
        if self._scratch is None or self._scratch.device != dev:
            # zeroed once: the narrowing pass clears what it reads, so the image is clean again after every call
            self._scratch = torch.zeros(self.bins * self.height * self.width, dtype=torch.int32, device=dev)
        out = torch.empty(self.get_shape(), dtype=torch.int8, device=dev)
        x, y, pol, time = (t.to(torch.int64).contiguous() for t in (x, y, pol, time))
        L.call('rvt_mixed_density_stack', L.ptr(x), L.ptr(y), L.ptr(pol), L.ptr(time), x.numel(), self.bins, self.height, self.width,
               -1 if self.count_cutoff is None else self.count_cutoff, L.ptr(self._scratch), L.ptr(out), L.stream_of(out))
        return out


_COORD_BYTES = {torch.int16: 2, torch.int32: 4, torch.int64: 8}
REPRESENTATIONS = ('stacked_histogram', 'mixed_density')
DEFAULT_WINDOWS_IN_FLIGHT = 8        # scratch images per chunk (profiles/evseq_bench.txt)
Stream = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


class EventTable:
    """The device stream table of one batch plus what it points at (the rows hold addresses: the tensors must stay alive)."""

    def __init__(self, dev: torch.Tensor, streams: List[Stream], ts_end: torch.Tensor, B: int, T: int, coord_bytes: int, capacity: int):
        self.dev, self.streams, self.ts_end, self.B, self.T, self.coord_bytes, self.capacity = dev, streams, ts_end, B, T, coord_bytes, capacity


class EventSequenceBuilder:
    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int] = None, fastmode: bool = True,
                 downsample_by_2: bool = False, window_us: Optional[int] = None, window_events: Optional[int] = None,
                 max_windows_in_flight: Optional[int] = None, representation: str = 'stacked_histogram', repair_time: bool = False):
        if representation not in REPRESENTATIONS:
            raise ValueError(f'representation={representation!r} is not one of {REPRESENTATIONS}')
        mixed = representation == 'mixed_density'
        if bins < 1 or height < 1 or width < 1:
            raise ValueError(f'bins={bins}, height={height}, width={width} must be positive')
        if (window_us is None) == (window_events is None):                 # preprocess_dataset.py: exactly one of the two
            raise ValueError(f'exactly one of window_us={window_us} and window_events={window_events} must be given')
        if (window_us if window_us is not None else window_events) < 1:
            raise ValueError(f'window_us={window_us} / window_events={window_events} must be positive')
        if downsample_by_2 and (height < 2 or width < 2):
            raise ValueError(f'downsample_by_2 needs height={height} and width={width} >= 2')
        if mixed:
            if fastmode is not True:
                raise ValueError(f'fastmode={fastmode} belongs to the stacked histogram: the mixed-density stack has no such mode')
            if count_cutoff is not None and not 0 <= count_cutoff <= 127:     # representations.py:140-142
                raise ValueError(f'count_cutoff={count_cutoff} must be None or 0..127 for the mixed-density stack')
        elif count_cutoff is not None and count_cutoff < 1:
            raise ValueError(f'count_cutoff={count_cutoff} must be >= 1')
        if max_windows_in_flight is not None and not 1 <= max_windows_in_flight <= 65535:
            raise ValueError(f'max_windows_in_flight={max_windows_in_flight} outside 1..65535')
        self.bins, self.height, self.width = bins, height, width
        self.representation, self.mixed = representation, mixed
        if mixed:
            self.count_cutoff = -1 if count_cutoff is None else int(count_cutoff)       # the C side's "no clamp"
        else:
            self.count_cutoff = 255 if count_cutoff is None else min(count_cutoff, 255)
        self.dtype = torch.int8 if mixed else torch.uint8
        self.fastmode, self.downsample_by_2 = bool(fastmode), bool(downsample_by_2)
        self.window_us, self.window_events = window_us, window_events
        self.max_windows_in_flight = max_windows_in_flight
        self.repair_time = bool(repair_time)
        self._scratch = None
        self._prep_ws = None

    def get_shape(self) -> Tuple[int, int, int]:
        """(2*bins, H', W') of one window, after the down-sampling; (bins, H', W') for the mixed-density stack."""
        C = self.bins if self.mixed else 2 * self.bins
        if self.downsample_by_2:
            return C, self.height // 2, self.width // 2
        return C, self.height, self.width

    # ---- the stream table
    def _host_table(self, streams: Sequence[Stream], ts_end: torch.Tensor, counts: Optional[Sequence[int]]):
        streams = [tuple(s) for s in streams]
        B = len(streams)
        if B < 1:
            raise ValueError('streams is empty')
        dev, cdt = ts_end.device, None
        rows = np.zeros(B, dtype=L.row_dtype('RvtEventStream'))
        capacity = 0
        for b, s in enumerate(streams):
            if len(s) != 4 or not all(torch.is_tensor(a) for a in s):
                raise TypeError(f'streams[{b}] must be a tuple (x, y, p, t) of tensors')
            x, y, p, t = s
            if t.dtype != torch.int64:
                raise TypeError(f'streams[{b}]: t must be int64 microseconds, got {t.dtype}')
            cdt = x.dtype if cdt is None else cdt
            if cdt not in _COORD_BYTES or any(a.dtype != cdt for a in (x, y, p)):
                raise TypeError(f'streams[{b}]: x, y, p must share one of int16 / int32 / int64 across the batch, '
                                f'got {x.dtype}, {y.dtype}, {p.dtype} (batch: {cdt})')
            for a in s:
                if a.dim() != 1 or a.numel() != t.numel() or a.device != dev:
                    raise ValueError(f'streams[{b}]: x, y, p, t must be 1-D tensors of one length on {dev}, got {tuple(a.shape)} on {a.device}')
            n = t.numel() if counts is None else int(counts[b])
            if not 0 <= n <= t.numel():
                raise ValueError(f'counts[{b}]={n} outside the buffers\' capacity 0..{t.numel()}')
            te = ts_end if ts_end.dim() == 1 else ts_end[b]
            row = rows[b]
            row['x'], row['y'], row['p'], row['t'], row['n'], row['ts_end'] = L.ptr(x), L.ptr(y), L.ptr(p), L.ptr(t), n, te.data_ptr()
            capacity = max(capacity, t.numel())
        return streams, rows.view(np.int64).reshape(B, -1), _COORD_BYTES[cdt], capacity

    @staticmethod
    def _check_ts_end(ts_end_us: torch.Tensor, B: int) -> torch.Tensor:
        if not torch.is_tensor(ts_end_us) or ts_end_us.dtype != torch.int64:
            raise TypeError(f'ts_end_us must be an int64 tensor, got {getattr(ts_end_us, "dtype", type(ts_end_us))}')
        if not (ts_end_us.dim() == 1 or (ts_end_us.dim() == 2 and ts_end_us.shape[0] == B)) or ts_end_us.shape[-1] < 1:
            raise ValueError(f'ts_end_us must be [T] or [B={B}][T] with T >= 1, got {tuple(ts_end_us.shape)}')
        if not ts_end_us.is_contiguous():
            raise ValueError('ts_end_us must be contiguous')
        return ts_end_us

    def make_table(self, streams: Sequence[Stream], ts_end_us: torch.Tensor, counts: Optional[Sequence[int]] = None) -> EventTable:
        """The device table of B streams.  counts[b]: events of stream b in use (default: the whole tensors)."""
        ts_end = self._check_ts_end(ts_end_us, len(streams))
        streams, rows, cb, cap = self._host_table(streams, ts_end, counts)
        return EventTable(torch.from_numpy(rows).to(ts_end.device), streams, ts_end, len(streams), int(ts_end.shape[-1]), cb, cap)

    def write_table(self, table: EventTable, streams: Optional[Sequence[Stream]] = None, ts_end_us: Optional[torch.Tensor] = None,
                    counts: Optional[Sequence[int]] = None) -> None:
        """Rewrite an existing device table in place (same address: a captured graph replays with the new streams / counts).
        streams / ts_end_us default to the table's own tensors, i.e. only the counts change."""
        streams = table.streams if streams is None else streams
        ts_end = table.ts_end if ts_end_us is None else self._check_ts_end(ts_end_us, len(streams))
        streams, rows, cb, cap = self._host_table(streams, ts_end, counts)
        if len(streams) != table.B or int(ts_end.shape[-1]) != table.T or cb != table.coord_bytes:
            raise ValueError(f'the table was made for B={table.B}, T={table.T}, {table.coord_bytes}-byte coordinates')
        table.dev.copy_(torch.from_numpy(rows))
        table.streams, table.ts_end, table.capacity = streams, ts_end, max(cap, table.capacity)

    # ---- the build
    def windows_in_flight(self, windows: int) -> int:
        return min(windows, self.max_windows_in_flight or DEFAULT_WINDOWS_IN_FLIGHT)

    def workspace(self, device, windows: int, B: Optional[int] = None) -> torch.Tensor:
        """The zeroed scratch images (the call keeps them zero); allocate ahead of a graph capture by calling this once.
        With repair_time, B streams: the repair's workspace as well."""
        if self.repair_time and B is not None and (self._prep_ws is None or not same_device(self._prep_ws.device, device)
                                                   or self._prep_ws.numel() < prep_ws_elems(B)):
            self._prep_ws = torch.empty(prep_ws_elems(B), dtype=torch.int64, device=device)
        C, H, W = self.get_shape()
        lib = L.get_lib()
        ws_bytes = lib.rvt_event_sequence_mixed_ws_bytes if self.mixed else lib.rvt_event_sequence_ws_bytes
        need = ws_bytes(self.bins, self.height, self.width, int(self.downsample_by_2), self.windows_in_flight(windows)) // 4
        if self._scratch is None or self._scratch.device != torch.device(device) or self._scratch.numel() < need:
            self._scratch = torch.zeros(need, dtype=torch.int32, device=device)
        return self._scratch

    def build_from_table(self, table: EventTable, out: Optional[torch.Tensor] = None, bounds_out: Optional[torch.Tensor] = None):
        B, T = table.B, table.T
        dev = table.dev.device
        shape = (T, B) + self.get_shape()
        if out is None:
            out = torch.empty(shape, dtype=self.dtype, device=dev)
        elif tuple(out.shape) != shape or out.dtype != self.dtype or out.device != dev or not out.is_contiguous():
            raise ValueError(f'out must be contiguous {str(self.dtype)[6:]} {shape} on {dev}, got {out.dtype} {tuple(out.shape)}')
        if bounds_out is None:
            bounds_out = torch.empty(B, T, 2, dtype=torch.int64, device=dev)
        elif tuple(bounds_out.shape) != (B, T, 2) or bounds_out.dtype != torch.int64 or bounds_out.device != dev or not bounds_out.is_contiguous():
            raise ValueError(f'bounds_out must be contiguous int64 {(B, T, 2)} on {dev}, got {bounds_out.dtype} {tuple(bounds_out.shape)}')
        scratch = self.workspace(dev, B * T, B)
        if self.repair_time:                                   # in place, no carry: every table is a whole stream
            L.call('rvt_event_time_repair', L.ptr(table.dev), B, None, None, L.ptr(self._prep_ws), 0, L.stream_of(out))
        # workgroups per window: the grid cannot follow bounds that live on the device, but never needs more than the capacity gives
        count_blocks = max(1, min(256, -(-table.capacity // 8192)))
        if self.mixed:
            L.call('rvt_event_sequence_mixed', L.ptr(table.dev), B, T, table.coord_bytes, self.window_us or 0, self.window_events or 0,
                   self.bins, self.height, self.width, int(self.downsample_by_2), self.count_cutoff, L.ptr(bounds_out), L.ptr(scratch),
                   self.windows_in_flight(B * T), count_blocks, L.ptr(out), L.stream_of(out))
            return out, bounds_out
        L.call('rvt_event_sequence', L.ptr(table.dev), B, T, table.coord_bytes, self.window_us or 0, self.window_events or 0, self.bins,
               self.height, self.width, int(self.downsample_by_2), self.count_cutoff, int(self.fastmode), L.ptr(bounds_out),
               L.ptr(scratch), self.windows_in_flight(B * T), count_blocks, L.ptr(out), L.stream_of(out))
        return out, bounds_out

    def build(self, streams: Sequence[Stream], ts_end_us: torch.Tensor, out: Optional[torch.Tensor] = None,
              bounds_out: Optional[torch.Tensor] = None):
        """streams: B tuples (x, y, p, t) of device tensors; ts_end_us int64 [T] or [B][T] -> (planes uint8 (T, B, C, H', W'),
        bounds int64 [B][T][2]); int8 planes for the mixed-density stack."""
        return self.build_from_table(self.make_table(streams, ts_end_us), out, bounds_out)


# ---- timestamp repair (rvt_amd/csrc/evprep.hpp)
def same_device(a, b) -> bool:
    """Do two device specifications name one device?  'cuda' without an index is the current device."""
    def resolve(d):
        d = torch.device(d)
        if d.type != 'cuda':
            return d.type, d.index or 0
        return d.type, torch.cuda.current_device() if d.index is None else d.index
    return resolve(a) == resolve(b)


def prep_ws_elems(B: int, blocks_per_stream: int = 0) -> int:
    """int64 elements of the workspace rvt_event_time_repair / rvt_event_decode_dat need for B streams."""
    n = L.get_lib().rvt_event_prep_ws_bytes(int(B), int(blocks_per_stream)) // 8
    if n < 1:
        raise ValueError(f'B={B}, blocks_per_stream={blocks_per_stream} out of range')
    return n


def prep_blocks(B: int, blocks_per_stream: int = 0) -> int:
    """Workgroups per stream of those entries (the second dimension of their ``repaired`` output)."""
    return prep_ws_elems(B, blocks_per_stream) // B - 1


def check_carry(carry: Optional[torch.Tensor], B: int, dev) -> None:
    if carry is not None and (not torch.is_tensor(carry) or carry.dtype != torch.int64 or tuple(carry.shape) != (B,) or carry.device != dev
                              or not carry.is_contiguous()):
        raise ValueError(f'carry must be a contiguous int64 [{B}] tensor on {dev}')


def repair_time(streams_or_table: Union[EventTable, Sequence[Stream]], carry: Optional[torch.Tensor] = None, out_repaired: bool = False,
                blocks_per_stream: int = 0, ws: Optional[torch.Tensor] = None):
    """Make the timestamps of B streams non-decreasing, in place: ``t[i] = max(c, t[0..i])`` with ``c = carry[b]``, or 0 without a
    carry (the reference reader's ``_correct_time``).  streams_or_table: B tuples ``(x, y, p, t)`` or an ``EventTable`` (its counts
    are honoured).  carry int64 ``[B]`` receives ``max(c, every t)``: chunks repaired one after the other with one carry equal the
    repair of the concatenated stream.  out_repaired: return int64 ``[B][K]`` counts of changed timestamps (sum over K per stream),
    else None.  ws: an int64 workspace of ``prep_ws_elems(B, blocks_per_stream)`` elements, for callers that capture a graph."""
    if isinstance(streams_or_table, EventTable):
        table = streams_or_table
    else:
        streams = [tuple(s) for s in streams_or_table]
        if not streams:
            raise ValueError('streams is empty')
        t0 = streams[0][3]
        # (the window ends are not read by the repair: any int64 tensor stands in for them)
        table = EventSequenceBuilder(1, 1, 1, window_us=1).make_table(streams, torch.zeros(1, dtype=torch.int64, device=t0.device))
    B, dev = table.B, table.dev.device
    check_carry(carry, B, dev)
    need = prep_ws_elems(B, blocks_per_stream)
    if ws is None:
        ws = torch.empty(need, dtype=torch.int64, device=dev)
    elif ws.dtype != torch.int64 or ws.numel() < need or ws.device != dev or not ws.is_contiguous():
        raise ValueError(f'ws must be a contiguous int64 tensor of at least {need} elements on {dev}')
    repaired = torch.empty(B, prep_blocks(B, blocks_per_stream), dtype=torch.int64, device=dev) if out_repaired else None
    L.call('rvt_event_time_repair', L.ptr(table.dev), B, L.ptr(carry), L.ptr(repaired), L.ptr(ws), int(blocks_per_stream),
           L.stream_of(table.dev))
    return repaired
