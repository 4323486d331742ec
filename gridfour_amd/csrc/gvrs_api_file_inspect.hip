// gvrs_api_file_inspect.hip -- GVRS files INSPECTED: gf_file_inspect_plan and gf_file_inspect (the walk of gvrs_file_inspect.h
// behind their argument checks; no device, no context) and gf_file_inspect_dev (the image in device memory walked and checksummed
// by the kernels of gvrs_file_inspect.hip, on the context's stream, enqueued only).
// Reference: gvrs/GvrsInspector.java:213-337.

#include "gvrs_api_internal.h"
#include "gvrs_file_inspect.h"

extern "C" {

gf_status gf_file_inspect_plan(const gf_file *f, size_t imageBytes, uint64_t *segmentBytes, uint64_t *crcChunkBytes, uint64_t *defaultMaxRecords)
{
    if (!f) return GF_ERR_ARG;
    gf_file_info info;
    const gf_status s = gf_file_get_info(f, &info);
    if (s != GF_OK) return s;
    gfInspectPlan(info, imageBytes, segmentBytes, crcChunkBytes, defaultMaxRecords);
    return GF_OK;
}

gf_status gf_file_inspect(const gf_file *f, const uint8_t *image, size_t imageBytes, gf_file_inspect_report *report, int32_t *badTiles, size_t badCap,
                          gf_file_record *records, size_t recordsCap)
{
    if (!f || !image || !report || (badCap && !badTiles)) return GF_ERR_ARG;
    gf_file_info info;
    const gf_status s = gf_file_get_info(f, &info);
    if (s != GF_OK) return s;
    return gfFileInspect(info, image, imageBytes, report, badTiles, badCap, records, recordsCap);
}

gf_status gf_file_inspect_dev(gf_context *c, const gf_file *f, const uint8_t *dImage, size_t imageBytes, size_t maxRecords,
                              gf_file_inspect_report *dReport, int32_t *dBadTiles, size_t badCap, gf_file_record *dRecords)
{
    if (!c || !f || !dImage || ((uintptr_t)dImage & 7) != 0 || !dReport || (badCap && !dBadTiles)) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    // (the header record's size word is the opened file's: the image's own is in device memory and is not read here)
    if ((s = gfInspectImageCheck(i, imageBytes, (uint32_t)(i.content_pos - 16))) != GF_OK) return s;
    uint64_t segBytes, chunk, defaultMax;
    gfInspectPlan(i, imageBytes, &segBytes, &chunk, &defaultMax);
    const uint64_t room = maxRecords ? maxRecords : std::max<uint64_t>(defaultMax, 1);
    if (room > 0x7ffffffeull) return GF_ERR_UNSUPPORTED;
    const uint64_t span = imageBytes - i.content_pos, nSeg = std::max<uint64_t>((span + segBytes - 1) / segBytes, 1);
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    // the context's part: state | the large records' sums || the anchors || landings | bases | counts | stops | the list | the large records
    Carve k;
    const size_t stateAt = k.add(sizeof(GfInspectState)), accAt = k.add((room + 1) * 4), zeroEnd = k.total;
    const size_t anchorAt = k.add(nSeg * 8), landingAt = k.add(nSeg * 8), baseAt = k.add(nSeg * 8), countAt = k.add(nSeg * 4), stopAt = k.add(nSeg * 4);
    const size_t recsAt = k.add((room + 1) * sizeof(gf_file_record)), largeAt = k.add((room + 1) * 4);
    if ((s = c->dFileInspect.ensure(k)) != GF_OK) return s;
    GfInspectArgs a{};
    a.image = dImage;
    a.p = gfInspectParamsOf(i, imageBytes);
    a.dir = gfFileDirOf(i), a.metaDirPos = i.metadata_dir_pos, a.freeDirPos = i.freespace_dir_pos;
    a.segBytes = segBytes, a.maxRecords = room, a.nSeg = (uint32_t)nSeg;
    a.state = c->dFileInspect.at<GfInspectState>(stateAt);
    a.acc = c->dFileInspect.at<uint32_t>(accAt);
    a.anchor = c->dFileInspect.at<uint64_t>(anchorAt), a.landing = c->dFileInspect.at<uint64_t>(landingAt), a.base = c->dFileInspect.at<uint64_t>(baseAt);
    a.count = c->dFileInspect.at<uint32_t>(countAt);
    a.stopc = c->dFileInspect.at<int32_t>(stopAt);
    a.recs = c->dFileInspect.at<gf_file_record>(recsAt);
    a.large = c->dFileInspect.at<uint32_t>(largeAt);
    a.report = dReport, a.badTiles = dBadTiles, a.badCap = badCap, a.records = dRecords;
    GF_HIP(hipMemsetAsync(a.state, 0, zeroEnd - stateAt, st));
    GF_HIP(hipMemsetAsync(a.anchor, 0xff, nSeg * 8, st));
    GF_HIP(gf_launch_file_inspect(a, st));
    return GF_OK;
}

}  // extern "C"
