"""The result-delivery contract of the four receive handles in plain Python, written from include/sora_hip.h's comments on sora_frame_result, *_results_of and
*_deliver_async.  It never reads the library: tests/test_deliver_model_cpu.py holds it to tables written out by hand, tests/test_gpu_deliver.py holds the handles
to it.  TEST INFRASTRUCTURE.

Input, everywhere: the call's captures in call order, each (capture_id, frames, mf) -- `frames` the frames FOUND in the capture in time order (there may be more
of them than rows), mf = max_frames_per_capture.  A frame is a dict of the row's fields (FIELDS; a missing one is 0) plus "mpdu": its bytes, or None.

The rules:
  - row order is (capture, time): the captures in call order, inside a capture the frames in time order;
  - the first min(found, mf) frames of a capture get rows;
  - SORA_ROW_TRUNCATED goes on row mf - 1 of a capture exactly when found > mf; the other flag bits (SORA_ROW_SHORT_PREAMBLE) pass through;
  - only E_FRAME_OK and E_CRC32_FAIL rows own bytes, min(length, 4096) of them;
  - deliver_async: mpdu_offset is the sum of the byte counts of all rows before it, whether or not those rows' bytes fitted, and whether or not there is an
    MPDU buffer at all; an MPDU is present exactly when offset + len <= mpdu_cap; counts = [rows, the total of the byte counts], not what fitted."""

E_FRAME_OK = 0x1
E_PLCP_HEADER_FAIL = 0x80000005
E_CRC32_FAIL = 0x80000006
ROW_TRUNCATED = 1
ROW_SHORT_PREAMBLE = 2
OK = 0
ERR_CAPACITY = -6
SLOT_BYTES = 32                                            # the 802.11a handle's MPDU array: 32 bytes per symbol slot
FIELDS = ("capture_id", "start_sample", "end_sample", "error_code", "rate_kbps", "length", "nsym", "crc32", "cfo_est", "flags", "mpdu_offset")


def owned(frame):
    """the bytes a row owns in the MPDU block: min(length, 4096) for E_FRAME_OK / E_CRC32_FAIL, else none"""
    return min(frame.get("length", 0), 4096) if frame.get("error_code", 0) in (E_FRAME_OK, E_CRC32_FAIL) else 0


def table(captures):
    """-> [(row without mpdu_offset, byte count, bytes or None)] in (capture, time) order"""
    out = []
    for capture_id, frames, mf in captures:
        for i, f in enumerate(frames[:mf]):
            row = {k: int(f.get(k, 0)) for k in FIELDS}
            row["capture_id"] = int(capture_id)
            row["flags"] |= ROW_TRUNCATED if i == mf - 1 and len(frames) > mf else 0
            n = owned(f)
            if n:
                assert f["mpdu"] is not None and len(f["mpdu"]) >= n, "a row that owns bytes needs them"
            out.append((row, n, bytes(f["mpdu"][:n]) if n else None))
    return out


def deliver(captures, mpdu_cap):
    """*_deliver_async of the 802.11b, 802.11n and 40 MHz HT handles.  mpdu_cap None: no MPDU buffer (h_mpdu NULL).
    -> {"rows", "counts": [rows, MPDU bytes], "present": per row, whether its MPDU is in the block, "mpdu": the dense block's defined prefix}.
    An MPDU that does not fit is left out; every later row's offset lies behind mpdu_cap then, so the bytes that are defined are a prefix of the block (a later
    row that owns no bytes is "present" with nothing)."""
    rows, present, block, off = [], [], bytearray(), 0
    for row, n, data in table(captures):
        row["mpdu_offset"] = off
        fits = mpdu_cap is not None and off + n <= mpdu_cap
        present.append(bool(n) and fits)
        if n and fits:
            assert len(block) == off
            block += data
        off += n
        rows.append(row)
    return {"rows": rows, "counts": [len(rows), off], "present": present, "mpdu": bytes(block)}


def results_of(captures, max_out, mpdu_cap):
    """sora_rx11b_results_of / sora_rx11n_results_of (and sora_rx_results_of, whose rows are the same walk over the packed table).  mpdu_cap None: h_mpdu NULL.
    -> {"rc", "rows": what `out` holds, "nout", "mpdu": the block's defined prefix}.
    What the header leaves open and the code does (stated in the header now):
      - mpdu_offset counts only bytes that were COPIED: with h_mpdu NULL every offset is 0, and a row behind one whose MPDU did not fit has that row's offset;
      - max_out short: the first max_out rows are written, *nout = max_out, SORA_ERR_CAPACITY;
      - mpdu_cap short: every row is still written; an MPDU that does not fit is skipped (a later, shorter one that fits is copied), SORA_ERR_CAPACITY."""
    rows, block, rc = [], bytearray(), OK
    for row, n, data in table(captures):
        if len(rows) >= max_out:
            rc = ERR_CAPACITY
            break
        row["mpdu_offset"] = len(block)
        rows.append(row)
        if mpdu_cap is not None and n:
            if len(block) + n > mpdu_cap:
                rc = ERR_CAPACITY
                continue
            block += data
    return {"rc": rc, "rows": rows, "nout": len(rows), "mpdu": bytes(block)}


def slots_11a(nsamples20):
    """symbol slots of a capture of nsamples20 samples at the 20 MHz rate: one per 80 samples begun, and one more"""
    return nsamples20 // 80 + 1


def deliver_11a(captures, nslots, max_rows, mpdu_bytes=None):
    """sora_rx_deliver_async.  There mpdu_offset indexes the handle's own MPDU array of sora_rx_mpdu_bytes() bytes: 32 bytes per symbol slot, capture k's slots
    behind those of the captures before it -- nslots[k] of them (slots_11a) -- and a frame's MPDU at the slot of its SIGNAL symbol, which starts behind the 144
    samples T11aLTS takes: slot (start_sample + 144) // 80 of its capture.  The position of a capture in the call is therefore an input.  mpdu_bytes: the size of h_mpdu, None for NULL; one smaller than the array is refused before anything is enqueued.
    -> {"rc"} when refused, else {"rc", "rows": the first max_rows at most, "nrows", "mpdu_bytes", "mpdus": [(offset, bytes)]}"""
    need = SLOT_BYTES * sum(nslots)
    if mpdu_bytes is not None and mpdu_bytes < need:
        return {"rc": ERR_CAPACITY}
    base, bases = 0, []
    for n in nslots:
        bases.append(base); base += n
    slots = [(f["start_sample"] + 144) // 80 for _, frames, mf in captures for f in frames[:mf]]
    of_capture = [k for k, (_, frames, mf) in enumerate(captures) for _ in frames[:mf]]
    rows, mpdus = [], []
    for (row, n, data), slot, k in zip(table(captures), slots, of_capture):
        assert 0 <= slot < nslots[k]
        row["mpdu_offset"] = SLOT_BYTES * (bases[k] + slot)
        rows.append(row)
        if n:
            mpdus.append((row["mpdu_offset"], data))
    return {"rc": OK, "rows": rows[:max_rows], "nrows": len(rows), "mpdu_bytes": need, "mpdus": mpdus}


# ---- the 40 MHz HT handle's tables as captures of the above ---------------------------------------------------------------------------------------------------------
def ht40_descriptor_call(frames, joint=False):
    """a descriptor call (sora_ht40_process_dev): frames [(frame_id, rate_kbps, nsym, [row per stream])], a row {error_code, length, crc32, mpdu} -> captures:
    two rows per frame, start_sample = the stream; one row per frame under joint coding.  Nothing is ever truncated."""
    per = 1 if joint else 2
    out = []
    for frame_id, rate, nsym, streams in frames:
        assert len(streams) == per
        out.append((frame_id, [dict(s, start_sample=k, rate_kbps=rate, nsym=nsym) for k, s in enumerate(streams)], per))
    return out


def ht40_capture_call(captures, joint=False):
    """a raw-capture call (sora_ht40_process_captures_dev): captures [(capture_id, events, mf)], an event {end_sample, error_code, rate_kbps (the MCS), nsym,
    "streams": [row per stream] or None for an event that ended in the front end} -> captures of the above, one per EVENT (the unit the delivery scans): a
    recorded frame gives two rows (one under joint coding) with start_sample = the stream, an event that ended in the front end one row with no bytes; all rows
    of event mf - 1 of a capture that raised more than mf carry SORA_ROW_TRUNCATED."""
    per = 1 if joint else 2
    out = []
    for capture_id, events, mf in captures:
        for i, e in enumerate(events[:mf]):
            flags = ROW_TRUNCATED if i == mf - 1 and len(events) > mf else 0
            if e.get("streams") is None:
                rows = [{"end_sample": e["end_sample"], "error_code": e["error_code"], "flags": flags}]
            else:
                assert len(e["streams"]) == per
                rows = [dict(s, start_sample=k, end_sample=e["end_sample"], rate_kbps=e["rate_kbps"], nsym=e["nsym"], flags=flags) for k, s in enumerate(e["streams"])]
            out.append((capture_id, rows, len(rows)))
    return out
