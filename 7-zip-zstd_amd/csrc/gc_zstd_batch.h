// gc_zstd_batch.h -- the batched zstd encoder (gpucodec.h "ZSTD, batched"; DESIGN.md section 4 "Batches"): N independent inputs of at most one block, one frame
// each, as N workgroups per stage in one launch set.  Included at the end of gc_api.hip: host code over the context and the stream encoder's workspace.
//
// What ties the stream encoder's kernels to "block b starts at b * 128 KiB of one stream" is how K1 finds its bytes and its end, how K3d, K4 and K5 take a block's
// length from the stream's size, and how K0x finds a frame.  Their batch forms (K1b gc_zstd_lz.hip, K3d / K4b / K5b gc_zstd_seq.hip / gc_zstd_frame.hip, K0x
// gc_xxh64.h) take an item table instead and share the bodies; K2, K3a-c run unchanged on the per-block workspace, block b of it holding item b of the round.
// An input of one block runs K1 at every level of the stream call (lz_frame_arg), so item i's bytes are the stream call's for that item alone.
//
// Rounds.  The workspace reserves a full block's rows whatever an item's size (workspace_resize), so a batch runs in rounds of at most R items through the same
// workspace, R = GC_BATCH_WS_BUDGET / bytes per block.  The rounds follow each other on the main stream; the output offset and the "too small" mark carry from one
// to the next in device memory (K4b), so the host reads nothing back in between.  Streams as in the stream call: finder on the main stream, sequences on stream2,
// literals on stream3, K0x -- ONE launch over all items -- on streamHash, joined in front of K4b.
#pragma once

#define GC_BATCH_WS_BUDGET (2ull << 30)      // bytes of per-block workspace a batch call may ask for: 1636 blocks of 1.3 MB, more than six times the CUs at one K1b workgroup per CU
#define GC_BT_EVENTS 6u                      // per round: finder start, finder end, sequences end (stream2), literals end (stream3), both joined, emit end

static void batch_release(gc_ctx* c)
{
    for (uint32_t i = 0; i < c->btEvRounds * GC_BT_EVENTS; i++) if (c->btEv[i]) hipEventDestroy(c->btEv[i]);
    free(c->btEv); c->btEv = nullptr; c->btEvRounds = 0;
    for (int i = 0; i < 3; i++) if (c->btEvCall[i]) { hipEventDestroy(c->btEvCall[i]); c->btEvCall[i] = nullptr; }
    if (c->btHostItems) hipHostFree(c->btHostItems);
    if (c->btHostStage) hipHostFree(c->btHostStage);
    c->btHostItems = nullptr; c->btHostStage = nullptr; c->btHostItemsCap = c->btHostStageCap = 0;
}

// items per round: what the budget holds, or test hook GC_BATCH_ROUND_ITEMS (a smaller number: several rounds on a small batch)
static uint32_t batch_round_items(gc_ctx* c)
{
    size_t perBlock = 0;
    workspace_resize(c, 0, &perBlock);
    uint32_t r = (uint32_t)(GC_BATCH_WS_BUDGET / perBlock);
    gc_env_u32("GC_BATCH_ROUND_ITEMS", 1u, r, &r);
    return r;
}

// pinned host memory of at least `need` bytes in *p (what it held is not carried over)
static int batch_host_reserve(void** p, size_t* cap, size_t need)
{
    if (need <= *cap) return GC_OK;
    if (*p) hipHostFree(*p);
    *p = nullptr; *cap = 0;
    if (hipHostMalloc(p, need) != hipSuccess) { *p = nullptr; return GC_ERR_NOMEM; }
    *cap = need;
    return GC_OK;
}

static int batch_events(gc_ctx* c, uint32_t nRounds)
{
    for (int i = 0; i < 3; i++) if (!c->btEvCall[i]) HIPCHK(c, hipEventCreate(&c->btEvCall[i]));
    if (nRounds <= c->btEvRounds) return GC_OK;
    hipEvent_t* ev = (hipEvent_t*)realloc(c->btEv, (size_t)nRounds * GC_BT_EVENTS * sizeof(hipEvent_t));
    if (!ev) { snprintf(c->err, sizeof(c->err), "no memory for the events of %u rounds", nRounds); return GC_ERR_NOMEM; }
    c->btEv = ev;
    for (uint32_t i = c->btEvRounds * GC_BT_EVENTS; i < nRounds * GC_BT_EVENTS; i++) c->btEv[i] = nullptr;
    for (uint32_t i = c->btEvRounds * GC_BT_EVENTS; i < nRounds * GC_BT_EVENTS; i++) {
        if (hipEventCreate(&c->btEv[i]) != hipSuccess) { c->btEv[i] = nullptr; c->btEvRounds = i / GC_BT_EVENTS + 1u; snprintf(c->err, sizeof(c->err), "hipEventCreate failed"); return GC_ERR_HIP; }
    }
    c->btEvRounds = nRounds;
    return GC_OK;
}

extern "C" size_t gc_zstd_batch_round_items(gc_ctx* c) { return c ? batch_round_items(c) : 0u; }

extern "C" size_t gc_zstd_batch_compress_bound(const gc_batch_item* items, size_t nItems)
{
    size_t b = 0;      // per item: 9 bytes of frame header at most, 3 of block header, the content stored raw, 4 of checksum
    for (size_t i = 0; items && i < nItems; i++) b += (size_t)items[i].src_size + GC_FRAME_OVERHEAD + 4u;
    return b;
}

extern "C" int gc_zstd_batch_compress_device(gc_ctx* c, const void* d_src, size_t srcBytes, const gc_batch_item* items, size_t nItems,
                                             void* d_dst, size_t dstCap, int level)
{
    if (!c) return GC_ERR_PARAM;
    if ((nItems && (!items || !d_dst)) || nItems > 0x7FFFFFFFu) { snprintf(c->err, sizeof(c->err), "batch: null table or destination, or more than 2^31 - 1 items"); return GC_ERR_PARAM; }
    for (size_t i = 0; i < nItems; i++) {
        const gc_batch_item& it = items[i];
        if (it.src_size > GC_ZSTD_BATCH_ITEM_MAX) {
            snprintf(c->err, sizeof(c->err), "batch item %zu has %u bytes: more than one block (%u); larger inputs take the stream calls", i, it.src_size, GC_ZSTD_BATCH_ITEM_MAX);
            return GC_ERR_PARAM;
        }
        if (it.src_off > srcBytes || it.src_size > srcBytes - it.src_off || (it.src_size && !d_src)) {
            snprintf(c->err, sizeof(c->err), "batch item %zu (offset %llu, %u bytes) ends behind the %zu bytes of the input", i, (unsigned long long)it.src_off, it.src_size, srcBytes);
            return GC_ERR_PARAM;
        }
    }
    (void)level;      // (one block: the block-local finder at every level, as in the stream call)
    HIPCHK(c, hipSetDevice(c->device));
    c->btTimed = false; c->btPending = false; c->btN = nItems; c->btRounds = 0;
    if (gc_buf_reserve(c->btResult, 16) != GC_OK) { snprintf(c->err, sizeof(c->err), "batch: no device memory"); return GC_ERR_NOMEM; }
    HIPCHK(c, hipMemsetAsync(c->btResult, 0, 16, c->stream));
    if (nItems == 0) { c->btPending = true; return GC_OK; }

    const uint32_t R = batch_round_items(c), n = (uint32_t)nItems;
    const uint32_t nRounds = (n + R - 1u) / R;
    int rc = ensure_workspace(c, n < R ? n : R);
    if (rc != GC_OK) return rc;
    if ((rc = batch_events(c, nRounds)) != GC_OK) return rc;
    if (nItems * sizeof(gc_batch_item) > c->btItems.cap || nItems * sizeof(gc_batch_result) > c->btResults.cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));      // (kernels of the last call may still read the old tables)
        if (gc_buf_reserve(c->btItems, nItems * sizeof(gc_batch_item)) != GC_OK || gc_buf_reserve(c->btResults, nItems * sizeof(gc_batch_result)) != GC_OK) {
            snprintf(c->err, sizeof(c->err), "device memory for the tables of %zu batch items failed", nItems); return GC_ERR_NOMEM; }
    }
    // the context's copy of the table: pinned, so the copy to the device is asynchronous and reads memory the caller no longer owns
    if (nItems * sizeof(gc_batch_item) > c->btHostItemsCap) HIPCHK(c, hipStreamSynchronize(c->stream));      // (the last call's copy may still be reading it)
    if (batch_host_reserve((void**)&c->btHostItems, &c->btHostItemsCap, nItems * sizeof(gc_batch_item)) != GC_OK) { snprintf(c->err, sizeof(c->err), "host memory for %zu batch items failed", nItems); return GC_ERR_NOMEM; }
    memcpy(c->btHostItems, items, nItems * sizeof(gc_batch_item));
    HIPCHK(c, hipMemcpyAsync(c->btItems, c->btHostItems, nItems * sizeof(gc_batch_item), hipMemcpyHostToDevice, c->stream));
    const uint8_t* src = (const uint8_t*)d_src;
    const gc_batch_item* dItems = c->btItems;
    HIPCHK(c, hipEventRecord(c->btEvCall[0], c->stream));
    const bool sums = c->optChecksum != 0u;
    if (sums) {       // K0x: all items in one launch, beside the rounds (the input and the table are ready where the main stream stands now)
        if (!c->streamHash) {
            if (hipStreamCreate(&c->streamHash) != hipSuccess) { c->streamHash = nullptr; snprintf(c->err, sizeof(c->err), "no stream for the content checksums"); return GC_ERR_HIP; }
            for (int i = 0; i < 2; i++) if (!c->evHash[i]) HIPCHK(c, hipEventCreate(&c->evHash[i]));
        }
        if (nItems * sizeof(uint64_t) > c->xxh.cap) {
            HIPCHK(c, hipStreamSynchronize(c->streamHash));
            if (gc_buf_reserve(c->xxh, nItems * sizeof(uint64_t)) != GC_OK) { snprintf(c->err, sizeof(c->err), "workspace allocation for %zu frame checksums failed", nItems); return GC_ERR_NOMEM; }
        }
        HIPCHK(c, hipStreamWaitEvent(c->streamHash, c->btEvCall[0], 0));
        GC_LAUNCH(gc_zstd_xxh64_batch_kernel, n, GC_XXH64_T, c->streamHash, src, dItems, c->xxh);
        HIPCHK(c, hipEventRecord(c->btEvCall[1], c->streamHash));
    }
    for (uint32_t r = 0; r < nRounds; r++) {
        const uint32_t i0 = r * R, m = n - i0 < R ? n - i0 : R;      // the round's items: i0 .. i0 + m, in blocks 0 .. m of the workspace
        const gc_batch_item* rItems = dItems + i0;
        hipEvent_t* ev = c->btEv + (size_t)r * GC_BT_EVENTS;
        HIPCHK(c, hipEventRecord(ev[0], c->stream));
        if (c->zdictSize) {      // K1b's dictionary variant: the context's dictionary as history in front of every item
            GC_LAUNCH(gc_zstd_lz_batch_dict_kernel, m, 1024, c->stream, src, rItems, (GcSeqRaw*)c->seqRaw, (uint8_t*)c->lit, (GcBlockMeta*)c->meta,
                      (const uint8_t*)c->zdict, c->zdictSize, (const uint32_t*)c->zdictTabL, (const uint32_t*)c->zdictTabS);
        } else {
            GC_LAUNCH(gc_zstd_lz_batch_kernel, m, 1024, c->stream, src, rItems, (GcSeqRaw*)c->seqRaw, (uint8_t*)c->lit, (GcBlockMeta*)c->meta);
        }
        HIPCHK(c, hipEventRecord(ev[1], c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, ev[1], 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream3, ev[1], 0));
        GC_LAUNCH(gc_zstd_seq_codes_kernel, m, GC_SEQ_T, c->stream2, (const GcSeqRaw*)c->seqRaw, (const GcBlockMeta*)c->meta, (uint64_t*)c->seqPacked, (uint32_t*)c->seqOff, (uint8_t*)c->codes,
                  (GcSeqHist*)c->seqHist, (uint8_t*)c->seqSec, (GcSectionInfo*)c->info, 1u, (unsigned long long*)nullptr);
        GC_LAUNCH(gc_zstd_seq_tables_kernel, m * 3u, 64, c->stream2, (const GcSeqHist*)c->seqHist, (const GcSectionInfo*)c->info, (GcSeqTabG*)c->seqTabs, (unsigned long long*)nullptr);
        GC_LAUNCH(gc_zstd_seq_chain_kernel, m * 3u, 64, c->stream2, (const uint8_t*)c->codes, (const GcSectionInfo*)c->info, (GcSeqTabG*)c->seqTabs, (uint16_t*)c->stOut, (unsigned long long*)nullptr);
        GC_LAUNCH(gc_zstd_seq_pack_batch_kernel, m, GC_SEQ_T, c->stream2, (const uint64_t*)c->seqPacked, (const uint8_t*)c->codes, (const uint16_t*)c->stOut, (const GcSeqTabG*)c->seqTabs,
                  (uint8_t*)c->seqSec, (GcSectionInfo*)c->info, rItems);
        HIPCHK(c, hipEventRecord(ev[2], c->stream2));
        GC_LAUNCH(gc_zstd_huf_kernel, m, 256, c->stream3, (const uint8_t*)c->lit, (const GcBlockMeta*)c->meta, (uint8_t*)c->litSec, (GcSectionInfo*)c->info);
        HIPCHK(c, hipEventRecord(ev[3], c->stream3));
        HIPCHK(c, hipStreamWaitEvent(c->stream, ev[2], 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream, ev[3], 0));
        if (sums && r == 0u) HIPCHK(c, hipStreamWaitEvent(c->stream, c->btEvCall[1], 0));      // K0x joins in front of the first K4b / K5b
        HIPCHK(c, hipEventRecord(ev[4], c->stream));
        GC_LAUNCH(gc_zstd_plan_batch_kernel, 1, 1024, c->stream, (const GcSectionInfo*)c->info, rItems, m, (uint64_t)dstCap, (GcFramePlan*)c->plan, c->btResults + i0,
                  (uint64_t*)c->btResult, sums ? 1u : 0u);
        GC_LAUNCH(gc_zstd_emit_batch_kernel, m, 256, c->stream, src, rItems, (const uint8_t*)c->litSec, (const uint8_t*)c->seqSec, (const GcSectionInfo*)c->info, (const GcFramePlan*)c->plan,
                  (const uint64_t*)c->btResult, (uint8_t*)d_dst, sums ? (const uint64_t*)(c->xxh + i0) : (const uint64_t*)nullptr);
        HIPCHK(c, hipEventRecord(ev[5], c->stream));
    }
    HIPCHK(c, hipEventRecord(c->btEvCall[2], c->stream));
    HIPCHK(c, hipGetLastError());
    c->btPending = true; c->btTimed = true; c->btRounds = nRounds;
    return GC_OK;
}

extern "C" int gc_zstd_batch_finish(gc_ctx* c, gc_batch_result* results, size_t* totalSize)
{
    if (!c) return GC_ERR_PARAM;
    if (!c->btPending) { snprintf(c->err, sizeof(c->err), "no batch call is pending"); return GC_ERR_PARAM; }
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t res[2] = { 0, 0 };
    HIPCHK(c, hipMemcpyAsync(res, c->btResult, 16, hipMemcpyDeviceToHost, c->stream));
    if (results && c->btN) HIPCHK(c, hipMemcpyAsync(results, c->btResults, c->btN * sizeof(gc_batch_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->btPending = false;
    if (res[1]) { snprintf(c->err, sizeof(c->err), "destination too small: need %llu bytes", (unsigned long long)res[0]); return GC_ERR_DST_SMALL; }
    if (totalSize) *totalSize = (size_t)res[0];
    return GC_OK;
}

extern "C" int gc_zstd_batch_compress_host(gc_ctx* c, const void* const* srcs, const size_t* sizes, size_t nItems, void* dst, size_t dstCap,
                                           int level, gc_batch_result* results, size_t* totalSize)
{
    if (!c) return GC_ERR_PARAM;
    if (nItems && (!srcs || !sizes)) { snprintf(c->err, sizeof(c->err), "batch: null item arrays"); return GC_ERR_PARAM; }
    HIPCHK(c, hipSetDevice(c->device));
    size_t inBytes = 0;
    for (size_t i = 0; i < nItems; i++) {
        if (sizes[i] > GC_ZSTD_BATCH_ITEM_MAX || (sizes[i] && !srcs[i])) {
            snprintf(c->err, sizeof(c->err), "batch item %zu has %zu bytes: more than one block (%u), or no data; larger inputs take the stream calls", i, sizes[i], GC_ZSTD_BATCH_ITEM_MAX);
            return GC_ERR_PARAM;
        }
        inBytes += sizes[i];
    }
    // gather: the items back to back in pinned memory, the table behind them (8-byte aligned)
    const size_t tabOff = (inBytes + 7u) & ~(size_t)7u;
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (a copy of the last call may still read the gather buffer)
    if (batch_host_reserve((void**)&c->btHostStage, &c->btHostStageCap, tabOff + nItems * sizeof(gc_batch_item) + 8u) != GC_OK) {
        snprintf(c->err, sizeof(c->err), "host memory for gathering %zu bytes failed", inBytes); return GC_ERR_NOMEM; }
    gc_batch_item* items = (gc_batch_item*)(c->btHostStage + tabOff);
    size_t off = 0;
    for (size_t i = 0; i < nItems; i++) {
        if (sizes[i]) memcpy(c->btHostStage + off, srcs[i], sizes[i]);
        items[i].src_off = off; items[i].src_size = (uint32_t)sizes[i]; items[i].reserved = 0;
        off += sizes[i];
    }
    const size_t bound = gc_zstd_batch_compress_bound(items, nItems);
    if (stage_reserve(c, inBytes, bound, 0u) != GC_OK) { snprintf(c->err, sizeof(c->err), "staging for a batch of %zu bytes failed", inBytes); return GC_ERR_NOMEM; }
    if (inBytes) HIPCHK(c, hipMemcpyAsync(c->dIn, c->btHostStage, inBytes, hipMemcpyHostToDevice, c->stream));      // ONE copy carries every input
    int rc = gc_zstd_batch_compress_device(c, c->dIn, inBytes, items, nItems, c->dOut, c->dOut.cap, level);
    if (rc != GC_OK) return rc;
    size_t total = 0;
    if ((rc = gc_zstd_batch_finish(c, results, &total)) != GC_OK) return rc;
    if (total > dstCap || (total && !dst)) { snprintf(c->err, sizeof(c->err), "destination too small: need %zu bytes", total); return GC_ERR_DST_SMALL; }
    if (total) { HIPCHK(c, hipMemcpyAsync(dst, c->dOut, total, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }      // ... and one every frame
    if (totalSize) *totalSize = total;
    return GC_OK;
}

// ms[0..2] = finder, entropy stages, plan + emit of the last batch call, summed over its rounds; ms[3] = first kernel start -> last kernel end
extern "C" int gc_zstd_batch_timing(gc_ctx* c, float ms[4])
{
    if (!c || !ms || !c->btTimed || c->btPending) return GC_ERR_PARAM;
    for (int i = 0; i < 3; i++) ms[i] = 0.f;
    for (uint32_t r = 0; r < c->btRounds; r++) {
        hipEvent_t* ev = c->btEv + (size_t)r * GC_BT_EVENTS;
        float t = 0.f;
        HIPCHK(c, hipEventElapsedTime(&t, ev[0], ev[1])); ms[0] += t;
        HIPCHK(c, hipEventElapsedTime(&t, ev[1], ev[4])); ms[1] += t;
        HIPCHK(c, hipEventElapsedTime(&t, ev[4], ev[5])); ms[2] += t;
    }
    HIPCHK(c, hipEventElapsedTime(&ms[3], c->btEvCall[0], c->btEvCall[2]));
    return GC_OK;
}

// ---- raw-content dictionaries (gpucodec.h "ZSTD, dictionaries"; DESIGN.md section 4 "Dictionaries") ----
#define GC_ZDICT_PAD 32u                     // zero bytes behind the dictionary: a 16-byte compare window that starts at its last byte stays inside the allocation
#define GC_ZDICT_TAB_BYTES ((size_t)4u << GC_ZDICT_LOG)     // one digest table of K1b's dictionary variant (gc_zstd_lz.hip)

extern "C" size_t gc_zstd_dictionary_size(gc_ctx* c) { return c ? c->zdictSize : 0u; }

extern "C" int gc_zstd_set_dictionary(gc_ctx* c, const void* dict, size_t n)
{
    if (!c) return GC_ERR_PARAM;
    if (n && !dict) { snprintf(c->err, sizeof(c->err), "dictionary: null pointer with %zu bytes", n); return GC_ERR_PARAM; }
    if (n && n < 8u) { snprintf(c->err, sizeof(c->err), "dictionary of %zu bytes: fewer than 8 bytes cannot be matched against (libzstd would ignore it)", n); return GC_ERR_PARAM; }
    if (n > GC_ZSTD_DICT_MAX) { snprintf(c->err, sizeof(c->err), "dictionary of %zu bytes: more than GC_ZSTD_DICT_MAX (%u)", n, GC_ZSTD_DICT_MAX); return GC_ERR_PARAM; }
    if (n) {
        const uint8_t* d = (const uint8_t*)dict;
        const uint32_t magic = (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
        if (magic == 0xEC30A437u) { snprintf(c->err, sizeof(c->err), "formatted dictionary (magic 0xEC30A437): only raw-content dictionaries are supported"); return GC_ERR_UNSUPPORTED; }
    }
    HIPCHK(c, hipSetDevice(c->device));
    // whatever is in flight finishes with the dictionary it was started with
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    HIPCHK(c, hipStreamSynchronize(c->stream3));
    if (c->streamHash) HIPCHK(c, hipStreamSynchronize(c->streamHash));
    c->zdictSize = 0;
    if (!n) return GC_OK;
    if (gc_buf_reserve(c->zdict, GC_ZSTD_DICT_MAX + GC_ZDICT_PAD) != GC_OK || gc_buf_reserve(c->zdictTabL, GC_ZDICT_TAB_BYTES) != GC_OK ||
        gc_buf_reserve(c->zdictTabS, GC_ZDICT_TAB_BYTES) != GC_OK) { snprintf(c->err, sizeof(c->err), "dictionary: no device memory"); return GC_ERR_NOMEM; }
    HIPCHK(c, hipMemsetAsync(c->zdict, 0, GC_ZSTD_DICT_MAX + GC_ZDICT_PAD, c->stream));
    HIPCHK(c, hipMemsetAsync(c->zdictTabL, 0, GC_ZDICT_TAB_BYTES, c->stream));
    HIPCHK(c, hipMemsetAsync(c->zdictTabS, 0, GC_ZDICT_TAB_BYTES, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->zdict, dict, n, hipMemcpyHostToDevice, c->stream));
    GC_LAUNCH(gc_zstd_dict_digest_kernel, ((uint32_t)n + 255u) / 256u, 256, c->stream, (const uint8_t*)c->zdict, (uint32_t)n, (uint32_t*)c->zdictTabL, (uint32_t*)c->zdictTabS);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (`dict` is the caller's again; the tables are read-only from here on)
    c->zdictSize = (uint32_t)n;
    return GC_OK;
}
