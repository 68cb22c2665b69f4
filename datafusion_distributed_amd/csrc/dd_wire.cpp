/* dd_wire.cpp — Arrow IPC *streaming format* + lz4 body compression for cross-node
 * (non-xGMI) hops. SURVEY.md §8(f) row 2.
 *
 * Replaces (by reimplementation, not translation) the reference's Flight encode path:
 * /root/reference/src/protocol/grpc/worker_service.rs:363-433 (FlightDataEncoder with
 * lz4-frame compression, arrow-ipc 59.2.0) and the decode at worker_client.rs:302. The
 * on-wire format is Apache Arrow's published IPC streaming format:
 *   [continuation 0xFFFFFFFF][meta_len i32][flatbuffer Message][pad8][body] ... [EOS]
 * with MetadataVersion V5 and per-buffer BodyCompression(LZ4_FRAME): each body buffer is
 * [i64 uncompressed_len][lz4-frame bytes], uncompressed_len = -1 meaning "stored raw"
 * (the spec's passthrough for incompressible buffers).
 *
 * The flatbuffers are built/read by a minimal hand-rolled builder (back-to-front with
 * distance-from-end alignment, exactly the flatbuffers wire layout) — no generated code,
 * no external flatbuffers dependency. Parity is pinned the only way that matters: blobs
 * we WRITE are read by pyarrow.ipc (an independent Arrow implementation), and blobs
 * pyarrow writes (compression="lz4") are read by us — tests/test_wire.py, including the
 * ZERO-COLUMN batches the reference wire-tests pin
 * (tests/empty_columns_between_workers.rs:11-31: RecordBatches that carry a row count
 * but no columns must survive the hop).
 *
 * lz4: the image ships the runtime library (liblz4.so.1, lz4 1.9.3) but no headers, so
 * the lz4frame ABI (stable since lz4 1.8) is declared here and resolved with dlopen.
 *
 * Types covered: u8/i16/i32/i64/f32/f64 (Int/FloatingPoint), bool (bit-packed on the
 * wire, unpacked u8 at this ABI like the device path), utf8 (i32 offsets + bytes).
 * Dictionary columns are exchanged as their indices + a materialized value column by
 * the host boundary (arrow_boundary.py); DictionaryBatch wire messages are out of this
 * tier's scope and return DD_ERR_UNSUPPORTED. */

#include <dlfcn.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "dd_shuffle.h"
#include "dd_internal.h"

/* ---------------- lz4frame ABI (resolved at runtime from liblz4.so.1) -------- */

namespace {

typedef size_t (*fn_compressFrameBound)(size_t, const void *);
typedef size_t (*fn_compressFrame)(void *, size_t, const void *, size_t, const void *);
typedef unsigned (*fn_isError)(size_t);
typedef size_t (*fn_createDCtx)(void **, unsigned);
typedef size_t (*fn_freeDCtx)(void *);
typedef size_t (*fn_decompress)(void *, void *, size_t *, const void *, size_t *,
                                const void *);

struct Lz4 {
    fn_compressFrameBound bound = nullptr;
    fn_compressFrame compress = nullptr;
    fn_isError is_error = nullptr;
    fn_createDCtx create_dctx = nullptr;
    fn_freeDCtx free_dctx = nullptr;
    fn_decompress decompress = nullptr;
    bool ok = false;
    Lz4() {
        void *h = dlopen("liblz4.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("liblz4.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        bound = (fn_compressFrameBound)dlsym(h, "LZ4F_compressFrameBound");
        compress = (fn_compressFrame)dlsym(h, "LZ4F_compressFrame");
        is_error = (fn_isError)dlsym(h, "LZ4F_isError");
        create_dctx = (fn_createDCtx)dlsym(h, "LZ4F_createDecompressionContext");
        free_dctx = (fn_freeDCtx)dlsym(h, "LZ4F_freeDecompressionContext");
        decompress = (fn_decompress)dlsym(h, "LZ4F_decompress");
        ok = bound && compress && is_error && create_dctx && free_dctx && decompress;
    }
};
Lz4 &lz4() {
    static Lz4 l;
    return l;
}
const unsigned LZ4F_VERSION_ABI = 100;

/* ---------------- minimal flatbuffer builder (back-to-front) ---------------- */

struct FB {
    std::vector<uint8_t> buf; /* built back-to-front; buf.size() = bytes written */
    size_t minalign = 8;

    size_t size() const { return buf.size(); }
    void fill(size_t n) { buf.insert(buf.end(), n, 0); }
    void prealign(size_t elem, size_t align) {
        if (align > minalign) minalign = align;
        size_t pad = (align - ((buf.size() + elem) % align)) % align;
        fill(pad);
    }
    void push_bytes(const void *p, size_t n) {
        const uint8_t *b = (const uint8_t *)p;
        /* back-to-front: reverse byte blocks, keep intra-block order */
        buf.insert(buf.end(), n, 0);
        uint8_t *dst = buf.data() + buf.size() - n;
        /* shift: everything previously written stays at the END in final order; we
         * model the final buffer as reverse(buf). Writing block b means appending
         * reverse(b) to buf. */
        for (size_t i = 0; i < n; i++) dst[i] = b[n - 1 - i];
    }
    template <typename T> size_t push(T v) {
        prealign(sizeof(T), sizeof(T));
        push_bytes(&v, sizeof(T));
        return size();
    }
    /* write a uoffset referring to `off` (an earlier finished object) */
    size_t push_ref(size_t off) {
        prealign(4, 4);
        uint32_t rel = (uint32_t)(size() - off + 4);
        push_bytes(&rel, 4);
        return size();
    }
    size_t make_string(const std::string &s) {
        /* the u32 length must IMMEDIATELY precede the bytes in the final buffer: pad so
         * that after NUL + bytes the write position is 4-aligned (accounting for the
         * CURRENT position), leaving push<u32> nothing to pad */
        fill((4 - ((buf.size() + s.size() + 1) % 4)) % 4);
        push_bytes("\0", 1);
        if (!s.empty()) push_bytes(s.data(), s.size());
        return push<uint32_t>((uint32_t)s.size());
    }
    size_t make_ref_vector(const std::vector<size_t> &offs) {
        prealign(4 * offs.size() + 4, 4);
        for (size_t i = offs.size(); i-- > 0;) {
            uint32_t rel = (uint32_t)(size() - offs[i] + 4);
            push_bytes(&rel, 4);
        }
        return push<uint32_t>((uint32_t)offs.size());
    }
    /* vector of 16-byte (i64,i64) structs; elements must land 8-aligned in the final
     * buffer: pad so the element block ends 8-aligned BEFORE the u32 length (which then
     * sits at final addr = 4 mod 8, putting element 0 at 0 mod 8) */
    size_t make_i64pair_vector(const std::vector<std::pair<int64_t, int64_t>> &v) {
        prealign(16 * v.size(), 8);
        for (size_t i = v.size(); i-- > 0;) {
            push_bytes(&v[i].second, 8);
            push_bytes(&v[i].first, 8);
        }
        size_t r = push<uint32_t>((uint32_t)v.size());
        return r;
    }

    /* table construction: collect (voffset_slot, position, size) then end_table */
    struct Table {
        struct F { uint16_t id; size_t pos; size_t sz; };
        std::vector<F> fields;
    };
    template <typename T> void add_scalar(Table &t, int id, T v, T dflt) {
        if (v == dflt) return;
        t.fields.push_back({(uint16_t)id, push<T>(v), sizeof(T)});
    }
    void add_ref(Table &t, int id, size_t off) {
        if (off == 0) return;
        t.fields.push_back({(uint16_t)id, push_ref(off), 4});
    }
    size_t end_table(Table &t) {
        size_t tableo = push<int32_t>(0); /* vtable soffset placeholder */
        int max_id = -1;
        for (auto &f : t.fields)
            if (f.id > max_id) max_id = f.id;
        uint16_t vt_len = (uint16_t)(4 + 2 * (max_id + 1));
        std::vector<uint16_t> vt(vt_len / 2, 0);
        vt[0] = vt_len;
        for (auto &f : t.fields) vt[2 + f.id] = (uint16_t)(tableo - f.pos);
        /* exact object size: distance from table start (soffset) to the farthest field
         * end. pos is the END-offset of the field; final extent = tableo - (pos - sz) */
        size_t obj = 4;
        for (auto &f : t.fields) {
            size_t ext = tableo - f.pos + f.sz;
            if (ext > obj) obj = ext;
        }
        vt[1] = (uint16_t)obj;
        prealign(vt_len, 2);
        for (size_t i = vt.size(); i-- > 0;) push_bytes(&vt[i], 2);
        size_t vto = size();
        /* patch soffset at tableo: final_addr(vtable) = N - vto; soffset = vto - tableo */
        int32_t so = (int32_t)(vto - tableo);
        /* tableo is distance-from-end of the END of the i32; its bytes live at
         * buf[tableo-4 .. tableo) in reversed storage => store reversed */
        uint8_t tmp[4];
        memcpy(tmp, &so, 4);
        for (int i = 0; i < 4; i++) buf[tableo - 1 - i] = tmp[i];
        return tableo;
    }

    /* finish: pad so total size is a multiple of minalign, push root ref, emit final */
    std::vector<uint8_t> finish(size_t root) {
        size_t total = size() + 4;
        size_t pad = (minalign - (total % minalign)) % minalign;
        fill(pad);
        push_ref(root);
        std::vector<uint8_t> out(buf.rbegin(), buf.rend());
        return out;
    }
};

/* ---------------- flatbuffer reader ---------------- */

struct FbTable {
    const uint8_t *base; /* buffer start */
    size_t len;
    size_t pos; /* table position; every accessor bounds-checks against len (the wire
                   may carry hostile/corrupt bytes — reads never leave the metadata
                   buffer; absent/invalid fields read as defaults) */

    bool valid() const { return pos != 0 && pos + 4 <= len; }
    uint16_t vt_entry(int id) const {
        if (!valid()) return 0;
        int32_t so;
        memcpy(&so, base + pos, 4);
        if (so < 0 ? pos + (size_t)(-so) > len : (size_t)so > pos) return 0;
        size_t vt = pos - so;
        if (vt + 4 > len) return 0;
        uint16_t vt_len;
        memcpy(&vt_len, base + vt, 2);
        if (vt_len < 4 || vt + vt_len > len) return 0;
        size_t slot = 4 + 2 * (size_t)id;
        if (slot + 2 > vt_len) return 0;
        uint16_t off;
        memcpy(&off, base + vt + slot, 2);
        return off;
    }
    template <typename T> T scalar(int id, T dflt) const {
        uint16_t o = vt_entry(id);
        if (!o || pos + o + sizeof(T) > len) return dflt;
        T v;
        memcpy(&v, base + pos + o, sizeof(T));
        return v;
    }
    size_t ref(int id) const { /* position of referenced object; 0 = absent/invalid */
        uint16_t o = vt_entry(id);
        if (!o || pos + o + 4 > len) return 0;
        uint32_t rel;
        memcpy(&rel, base + pos + o, 4);
        size_t t = pos + o + rel;
        return (t + 4 <= len) ? t : 0;
    }
    FbTable table(int id) const { return FbTable{base, len, ref(id)}; }
};


struct FbVector {
    const uint8_t *base;
    size_t pos; /* 0 = absent */
    size_t len = SIZE_MAX; /* metadata buffer bound (when provided) */
    uint32_t count() const {
        if (!pos || pos + 4 > len) return 0;
        uint32_t n;
        memcpy(&n, base + pos, 4);
        /* clamp: a hostile count cannot push element reads past the buffer */
        if (len != SIZE_MAX && pos + 4 + (size_t)n * 4 > len && n > (len - pos) / 4)
            n = (uint32_t)((len - pos - 4) / 4);
        return n;
    }
    size_t elem(size_t i, size_t elem_size) const { return pos + 4 + i * elem_size; }
    size_t ref_elem(size_t i) const {
        size_t e = elem(i, 4);
        if (e + 4 > len) return 0;
        uint32_t rel;
        memcpy(&rel, base + e, 4);
        return e + rel;
    }
};

/* ---------------- Arrow IPC constants ---------------- */

enum { MSG_SCHEMA = 1, MSG_DICTBATCH = 2, MSG_RECORDBATCH = 3 };
enum { TYPE_NULL = 1, TYPE_INT = 2, TYPE_FP = 3, TYPE_BINARY = 4, TYPE_UTF8 = 5,
       TYPE_BOOL = 6, TYPE_DATE = 8 };
const int16_t METADATA_V5 = 4;
const int8_t CODEC_LZ4_FRAME = 0;

struct WireCol {
    int32_t dtype; /* dd_dtype */
    std::string name;
    int32_t nullable;
};

size_t fb_field(FB &fb, const WireCol &c) {
    /* type table first */
    FB::Table tt;
    size_t type_off = 0;
    uint8_t type_type = 0;
    switch (c.dtype) {
    case DD_DT_U8: {
        FB::Table t;
        fb.add_scalar<int32_t>(t, 0, 8, 0);       /* bitWidth */
        fb.add_scalar<uint8_t>(t, 1, 0, 0);       /* is_signed=false */
        type_off = fb.end_table(t);
        type_type = TYPE_INT;
        break;
    }
    case DD_DT_I16:
    case DD_DT_I32:
    case DD_DT_I64: {
        FB::Table t;
        int bw = c.dtype == DD_DT_I16 ? 16 : c.dtype == DD_DT_I32 ? 32 : 64;
        fb.add_scalar<int32_t>(t, 0, bw, 0);
        fb.add_scalar<uint8_t>(t, 1, 1, 0); /* signed */
        type_off = fb.end_table(t);
        type_type = TYPE_INT;
        break;
    }
    case DD_DT_F32:
    case DD_DT_F64: {
        FB::Table t;
        fb.add_scalar<int16_t>(t, 0, c.dtype == DD_DT_F32 ? 1 : 2, 0); /* precision */
        type_off = fb.end_table(t);
        type_type = TYPE_FP;
        break;
    }
    case DD_DT_BOOL: {
        FB::Table t;
        type_off = fb.end_table(t);
        type_type = TYPE_BOOL;
        break;
    }
    case DD_DT_UTF8: {
        FB::Table t;
        type_off = fb.end_table(t);
        type_type = TYPE_UTF8;
        break;
    }
    default:
        return 0;
    }
    size_t name_off = fb.make_string(c.name);
    size_t children = fb.make_ref_vector({});
    FB::Table f;
    /* build in reverse-dependency order is already done; table slots: */
    fb.add_ref(f, 0, name_off);
    fb.add_scalar<uint8_t>(f, 1, (uint8_t)(c.nullable ? 1 : 0), 0);
    fb.add_scalar<uint8_t>(f, 2, type_type, 0);
    fb.add_ref(f, 3, type_off);
    fb.add_ref(f, 5, children);
    return fb.end_table(f);
}

std::vector<uint8_t> encap(const std::vector<uint8_t> &flat) {
    /* [0xFFFFFFFF][meta_len][flatbuffer][pad to 8] */
    size_t meta = flat.size();
    size_t padded = (meta + 7) & ~(size_t)7;
    std::vector<uint8_t> out(8 + padded, 0);
    out[0] = out[1] = out[2] = out[3] = 0xFF;
    int32_t ml = (int32_t)padded;
    memcpy(out.data() + 4, &ml, 4);
    memcpy(out.data() + 8, flat.data(), meta);
    return out;
}

} // namespace

/* ---------------- writer ---------------- */

struct dd_ipc_writer {
    std::vector<WireCol> cols;
    int use_lz4 = 0;
    std::vector<uint8_t> out;
    bool finished = false;
    std::string err;
};

extern "C" dd_status dd_ipc_writer_create(const dd_ipc_field *fields, int32_t n_fields,
                                          int32_t use_lz4, dd_ipc_writer **outw) {
    if ((!fields && n_fields > 0) || n_fields < 0 || !outw)
        return dd_set_error(DD_ERR_INVALID, "null argument");
    if (use_lz4 && !lz4().ok)
        return dd_set_error(DD_ERR_UNSUPPORTED, "liblz4.so.1 not resolvable");
    auto w = new dd_ipc_writer();
    w->use_lz4 = use_lz4;
    for (int32_t i = 0; i < n_fields; i++) {
        if (fields[i].dtype == DD_DT_DICT32) {
            delete w;
            return dd_set_error(DD_ERR_UNSUPPORTED,
                                "dictionary columns cross the wire as indices + values "
                                "(arrow_boundary); DictionaryBatch messages are out of "
                                "tier scope");
        }
        if (fields[i].dtype == DD_DT_DEC128) {
            delete w;
            return dd_set_error(DD_ERR_UNSUPPORTED,
                                "dec128 columns are not on the wire: dd_ipc_field carries no "
                                "precision and scale (DESIGN.md §16)");
        }
        w->cols.push_back({fields[i].dtype,
                           fields[i].name ? fields[i].name : ("f" + std::to_string(i)),
                           fields[i].nullable});
    }
    /* schema message */
    FB fb;
    std::vector<size_t> foffs;
    for (auto &c : w->cols) {
        size_t f = fb_field(fb, c);
        if (!f) {
            delete w;
            return dd_set_error(DD_ERR_UNSUPPORTED, "unsupported wire dtype");
        }
        foffs.push_back(f);
    }
    FB::Table sc;
    size_t fvec = fb.make_ref_vector(foffs);
    fb.add_scalar<int16_t>(sc, 0, 0, 0); /* endianness little */
    fb.add_ref(sc, 1, fvec);
    size_t schema = fb.end_table(sc);
    FB::Table msg;
    fb.add_scalar<int16_t>(msg, 0, METADATA_V5, 0);
    fb.add_scalar<uint8_t>(msg, 1, MSG_SCHEMA, 0);
    fb.add_ref(msg, 2, schema);
    /* bodyLength 0 default */
    size_t m = fb.end_table(msg);
    auto flat = fb.finish(m);
    w->out = encap(flat);
    *outw = w;
    return DD_OK;
}

static void pack_bits(const uint8_t *u8, int64_t n, std::vector<uint8_t> &out) {
    out.assign((size_t)((n + 7) / 8), 0);
    for (int64_t i = 0; i < n; i++)
        if (u8[i]) out[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
}

extern "C" dd_status dd_ipc_writer_batch(dd_ipc_writer *w, int64_t n_rows,
                                         const dd_ipc_array *cols) {
    if (!w || n_rows < 0 || (!cols && !w->cols.empty()))
        return dd_set_error(DD_ERR_INVALID, "null argument");
    if (w->finished) return dd_set_error(DD_ERR_INVALID, "writer already finished");

    struct Buf {
        std::vector<uint8_t> owned; /* packed bits / compressed */
        const uint8_t *p;
        size_t n;
    };
    std::vector<Buf> bufs;
    std::vector<std::pair<int64_t, int64_t>> nodes; /* FieldNode: length, null_count */

    auto add_raw = [&](const void *p, size_t n) {
        bufs.push_back({{}, (const uint8_t *)p, n});
    };
    std::vector<std::vector<uint8_t>> scratch; /* keeps packed bitmaps alive */

    for (size_t i = 0; i < w->cols.size(); i++) {
        const WireCol &c = w->cols[i];
        const dd_ipc_array &a = cols[i];
        nodes.push_back({n_rows, a.null_count});
        /* validity: unpacked u8 at this ABI -> packed bits on the wire */
        if (a.validity && a.null_count > 0) {
            scratch.emplace_back();
            pack_bits(a.validity, n_rows, scratch.back());
            add_raw(scratch.back().data(), scratch.back().size());
        } else {
            add_raw(nullptr, 0);
        }
        if (c.dtype == DD_DT_UTF8) {
            add_raw(a.offsets, (size_t)(n_rows + 1) * 4);
            add_raw(a.data, (size_t)a.data_len);
        } else if (c.dtype == DD_DT_BOOL) {
            scratch.emplace_back();
            pack_bits((const uint8_t *)a.data, n_rows, scratch.back());
            add_raw(scratch.back().data(), scratch.back().size());
        } else {
            size_t elem = c.dtype == DD_DT_U8 ? 1
                          : c.dtype == DD_DT_I16 ? 2
                          : (c.dtype == DD_DT_I32 || c.dtype == DD_DT_F32) ? 4 : 8;
            add_raw(a.data, (size_t)n_rows * elem);
        }
    }

    /* body: per buffer, 8-aligned; lz4: [i64 uncompressed][frame] with -1 passthrough */
    std::vector<uint8_t> body;
    std::vector<std::pair<int64_t, int64_t>> bvec; /* Buffer: offset, length */
    for (auto &b : bufs) {
        size_t start = body.size();
        if (b.n == 0) {
            bvec.push_back({(int64_t)start, 0});
            continue;
        }
        if (w->use_lz4) {
            size_t bound = lz4().bound(b.n, nullptr);
            std::vector<uint8_t> comp(bound);
            size_t cn = lz4().compress(comp.data(), bound, b.p, b.n, nullptr);
            if (lz4().is_error(cn))
                return dd_set_error(DD_ERR_INVALID, "lz4 compression failed");
            int64_t hdr;
            const uint8_t *payload;
            size_t pn;
            if (cn >= b.n) { /* incompressible: spec passthrough, hdr = -1 */
                hdr = -1;
                payload = b.p;
                pn = b.n;
            } else {
                hdr = (int64_t)b.n;
                payload = comp.data();
                pn = cn;
            }
            body.insert(body.end(), (uint8_t *)&hdr, (uint8_t *)&hdr + 8);
            body.insert(body.end(), payload, payload + pn);
            bvec.push_back({(int64_t)start, (int64_t)(8 + pn)});
        } else {
            body.insert(body.end(), b.p, b.p + b.n);
            bvec.push_back({(int64_t)start, (int64_t)b.n});
        }
        body.resize((body.size() + 7) & ~(size_t)7, 0);
    }

    FB fb;
    size_t comp_off = 0;
    if (w->use_lz4) {
        FB::Table ct;
        fb.add_scalar<int8_t>(ct, 0, CODEC_LZ4_FRAME, -1); /* default is 0: force-write */
        comp_off = fb.end_table(ct);
    }
    size_t nvec = fb.make_i64pair_vector(nodes);
    size_t bv = fb.make_i64pair_vector(bvec);
    FB::Table rb;
    fb.add_scalar<int64_t>(rb, 0, n_rows, -1); /* force-write length (0 rows is valid) */
    fb.add_ref(rb, 1, nvec);
    fb.add_ref(rb, 2, bv);
    fb.add_ref(rb, 3, comp_off);
    size_t rbo = fb.end_table(rb);
    FB::Table msg;
    fb.add_scalar<int16_t>(msg, 0, METADATA_V5, 0);
    fb.add_scalar<uint8_t>(msg, 1, MSG_RECORDBATCH, 0);
    fb.add_ref(msg, 2, rbo);
    fb.add_scalar<int64_t>(msg, 3, (int64_t)body.size(), 0);
    size_t m = fb.end_table(msg);
    auto flat = fb.finish(m);
    auto env = encap(flat);
    w->out.insert(w->out.end(), env.begin(), env.end());
    w->out.insert(w->out.end(), body.begin(), body.end());
    return DD_OK;
}

extern "C" dd_status dd_ipc_writer_finish(dd_ipc_writer *w, const uint8_t **data,
                                          int64_t *len) {
    if (!w || !data || !len) return dd_set_error(DD_ERR_INVALID, "null argument");
    if (!w->finished) {
        const uint8_t eos[8] = {0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0};
        w->out.insert(w->out.end(), eos, eos + 8);
        w->finished = true;
    }
    *data = w->out.data();
    *len = (int64_t)w->out.size();
    return DD_OK;
}

extern "C" void dd_ipc_writer_destroy(dd_ipc_writer *w) { delete w; }

/* ---------------- reader ---------------- */

struct dd_ipc_reader {
    std::vector<WireCol> cols;
    struct Batch {
        int64_t n_rows;
        /* per column: materialized buffers (decompressed, validity unpacked to u8) */
        std::vector<std::vector<uint8_t>> validity; /* unpacked u8, empty = all valid */
        std::vector<std::vector<uint8_t>> data;
        std::vector<std::vector<uint8_t>> offsets;
        std::vector<int64_t> null_count;
    };
    std::vector<Batch> batches;
};

namespace {

bool decompress_buf(const uint8_t *p, size_t n, int compressed, std::vector<uint8_t> &out) {
    if (!compressed) {
        out.assign(p, p + n);
        return true;
    }
    if (n < 8) return n == 0; /* empty buffer stays empty */
    int64_t ulen;
    memcpy(&ulen, p, 8);
    if (ulen == -1) {
        out.assign(p + 8, p + n);
        return true;
    }
    /* hostile-length guard: lz4 frames expand at most ~255x (+ header slack); a claimed
     * size beyond that is corrupt — refuse instead of attempting a huge allocation */
    if (ulen < 0 || (uint64_t)ulen > (uint64_t)(n - 8) * 256 + 65536) return false;
    out.resize((size_t)ulen);
    if (ulen == 0) return true;
    void *dctx = nullptr;
    if (lz4().is_error(lz4().create_dctx(&dctx, LZ4F_VERSION_ABI))) return false;
    size_t dst_n = (size_t)ulen, src_n = n - 8;
    size_t r = lz4().decompress(dctx, out.data(), &dst_n, p + 8, &src_n, nullptr);
    lz4().free_dctx(dctx);
    return !lz4().is_error(r) && dst_n == (size_t)ulen;
}

void unpack_bits(const uint8_t *bits, int64_t n, std::vector<uint8_t> &out) {
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; i++)
        out[(size_t)i] = (bits[(size_t)(i >> 3)] >> (i & 7)) & 1;
}

int32_t field_dtype(const FbTable &f) {
    uint8_t tt = f.scalar<uint8_t>(2, 0);
    FbTable ty = f.table(3);
    switch (tt) {
    case TYPE_INT: {
        int32_t bw = ty.valid() ? ty.scalar<int32_t>(0, 0) : 0;
        uint8_t sg = ty.valid() ? ty.scalar<uint8_t>(1, 0) : 0;
        if (bw == 8) return DD_DT_U8; /* both signednesses land on the 1-byte lane */
        if (bw == 16) return DD_DT_I16;
        if (bw == 32) return DD_DT_I32;
        if (bw == 64) return DD_DT_I64;
        (void)sg;
        return 0;
    }
    case TYPE_FP: {
        int16_t prec = ty.valid() ? ty.scalar<int16_t>(0, 0) : 0;
        if (prec == 1) return DD_DT_F32;
        if (prec == 2) return DD_DT_F64;
        return 0;
    }
    case TYPE_BOOL:
        return DD_DT_BOOL;
    case TYPE_UTF8:
        return DD_DT_UTF8;
    case TYPE_DATE: { /* Date32(DAY) decodes onto the i32 lane */
        int16_t unit = ty.valid() ? ty.scalar<int16_t>(0, 0) : 0;
        return unit == 0 ? DD_DT_I32 : 0;
    }
    default:
        return 0;
    }
}

} // namespace

extern "C" dd_status dd_ipc_reader_create(const uint8_t *data, int64_t len,
                                          dd_ipc_reader **outr) {
    if (!data || len < 8 || !outr) return dd_set_error(DD_ERR_INVALID, "null argument");
    auto r = std::unique_ptr<dd_ipc_reader>(new dd_ipc_reader());
    size_t pos = 0;
    bool have_schema = false;
    while (pos + 8 <= (size_t)len) {
        uint32_t cont;
        memcpy(&cont, data + pos, 4);
        int32_t meta_len;
        size_t meta_at;
        if (cont == 0xFFFFFFFFu) {
            memcpy(&meta_len, data + pos + 4, 4);
            meta_at = pos + 8;
        } else { /* legacy un-continued framing */
            memcpy(&meta_len, data + pos, 4);
            meta_at = pos + 4;
        }
        if (meta_len == 0) break; /* EOS */
        if (meta_len < 8 || meta_at + (size_t)meta_len > (size_t)len)
            return dd_set_error(DD_ERR_INVALID, "truncated IPC message");
        const uint8_t *flat = data + meta_at;
        uint32_t rootrel;
        memcpy(&rootrel, flat, 4);
        FbTable msg{flat, (size_t)meta_len, rootrel};
        uint8_t hdr_type = msg.scalar<uint8_t>(1, 0);
        const int64_t body_len = msg.scalar<int64_t>(3, 0);
        const uint8_t *body = data + meta_at + meta_len;
        if (body_len < 0 || meta_at + meta_len + (size_t)body_len > (size_t)len)
            return dd_set_error(DD_ERR_INVALID, "truncated IPC body");

        if (hdr_type == MSG_SCHEMA) {
            FbTable schema = msg.table(2);
            FbVector fields{flat, schema.ref(1), (size_t)meta_len};
            for (uint32_t i = 0; i < fields.count(); i++) {
                FbTable f{flat, (size_t)meta_len, fields.ref_elem(i)};
                if (f.ref(4) != 0)
                    return dd_set_error(DD_ERR_UNSUPPORTED,
                                        "dictionary-encoded wire fields are out of "
                                        "tier scope");
                int32_t dt = field_dtype(f);
                if (!dt) return dd_set_error(DD_ERR_UNSUPPORTED, "unsupported wire type");
                std::string name;
                size_t nm = f.ref(0);
                if (nm && nm + 4 <= (size_t)meta_len) {
                    uint32_t nl;
                    memcpy(&nl, flat + nm, 4);
                    if (nm + 4 + (size_t)nl <= (size_t)meta_len) /* hostile-length guard */
                        name.assign((const char *)flat + nm + 4, nl);
                }
                r->cols.push_back({dt, name, (int32_t)f.scalar<uint8_t>(1, 0)});
            }
            have_schema = true;
        } else if (hdr_type == MSG_RECORDBATCH) {
            if (!have_schema)
                return dd_set_error(DD_ERR_INVALID, "RecordBatch before Schema");
            FbTable rb = msg.table(2);
            int64_t n_rows = rb.scalar<int64_t>(0, 0);
            /* hostile row-count guard: rows must be representable by the stream's own
             * buffers (validity/bool checks below bound further) */
            if (n_rows < 0 || (uint64_t)n_rows > (uint64_t)len * 256 + 65536)
                return dd_set_error(DD_ERR_INVALID, "implausible row count");
            FbVector nodes{flat, rb.ref(1), (size_t)meta_len};
            FbVector buffers{flat, rb.ref(2), (size_t)meta_len};
            int compressed = 0;
            FbTable comp = rb.table(3);
            if (comp.valid()) {
                if (comp.scalar<int8_t>(0, 0) != CODEC_LZ4_FRAME)
                    return dd_set_error(DD_ERR_UNSUPPORTED, "only LZ4_FRAME compression");
                if (!lz4().ok)
                    return dd_set_error(DD_ERR_UNSUPPORTED, "liblz4.so.1 not resolvable");
                compressed = 1;
            }
            dd_ipc_reader::Batch bt;
            bt.n_rows = n_rows;
            size_t bi = 0;
            auto next_buf = [&](std::vector<uint8_t> &out) -> bool {
                if (bi >= buffers.count()) return false;
                int64_t off, blen;
                size_t e = buffers.elem(bi++, 16);
                if (e + 16 > (size_t)meta_len) return false;
                memcpy(&off, flat + e, 8);
                memcpy(&blen, flat + e + 8, 8);
                if (off < 0 || blen < 0 || off + blen > body_len) return false;
                return decompress_buf(body + off, (size_t)blen, compressed, out);
            };
            for (size_t c = 0; c < r->cols.size(); c++) {
                int64_t nc = 0;
                if (c < nodes.count()) {
                    size_t e = nodes.elem(c, 16);
                    if (e + 16 <= (size_t)meta_len) memcpy(&nc, flat + e + 8, 8);
                }
                bt.null_count.push_back(nc);
                std::vector<uint8_t> vbits, dat, off;
                if (!next_buf(vbits))
                    return dd_set_error(DD_ERR_INVALID, "missing validity buffer");
                std::vector<uint8_t> vu8;
                if (!vbits.empty() && nc > 0) {
                    if ((int64_t)vbits.size() * 8 < n_rows)
                        return dd_set_error(DD_ERR_INVALID, "validity bitmap too short");
                    unpack_bits(vbits.data(), n_rows, vu8);
                }
                bt.validity.push_back(std::move(vu8));
                if (r->cols[c].dtype == DD_DT_UTF8) {
                    if (!next_buf(off) || !next_buf(dat))
                        return dd_set_error(DD_ERR_INVALID, "missing utf8 buffers");
                    if ((int64_t)off.size() < (n_rows + 1) * 4)
                        return dd_set_error(DD_ERR_INVALID, "utf8 offsets too short");
                } else if (r->cols[c].dtype == DD_DT_BOOL) {
                    std::vector<uint8_t> bits;
                    if (!next_buf(bits))
                        return dd_set_error(DD_ERR_INVALID, "missing bool buffer");
                    if ((int64_t)bits.size() * 8 < n_rows)
                        return dd_set_error(DD_ERR_INVALID, "bool bitmap too short");
                    unpack_bits(bits.data(), n_rows, dat);
                } else {
                    if (!next_buf(dat))
                        return dd_set_error(DD_ERR_INVALID, "missing data buffer");
                }
                bt.data.push_back(std::move(dat));
                bt.offsets.push_back(std::move(off));
            }
            r->batches.push_back(std::move(bt));
        } else if (hdr_type == MSG_DICTBATCH) {
            return dd_set_error(DD_ERR_UNSUPPORTED, "DictionaryBatch is out of tier scope");
        } /* other message types skipped */
        pos = meta_at + meta_len + (size_t)body_len;
    }
    if (!have_schema) return dd_set_error(DD_ERR_INVALID, "no Schema message");
    *outr = r.release();
    return DD_OK;
}

extern "C" int32_t dd_ipc_reader_n_fields(const dd_ipc_reader *r) {
    return (int32_t)r->cols.size();
}
extern "C" int32_t dd_ipc_reader_n_batches(const dd_ipc_reader *r) {
    return (int32_t)r->batches.size();
}
extern "C" int32_t dd_ipc_reader_field_dtype(const dd_ipc_reader *r, int32_t i) {
    return r->cols[(size_t)i].dtype;
}
extern "C" const char *dd_ipc_reader_field_name(const dd_ipc_reader *r, int32_t i) {
    return r->cols[(size_t)i].name.c_str();
}
extern "C" int64_t dd_ipc_reader_batch_rows(const dd_ipc_reader *r, int32_t b) {
    return r->batches[(size_t)b].n_rows;
}
extern "C" dd_status dd_ipc_reader_batch_col(const dd_ipc_reader *r, int32_t b,
                                             int32_t c, dd_ipc_array *out) {
    if (!r || !out || b < 0 || b >= (int32_t)r->batches.size() || c < 0 ||
        c >= (int32_t)r->cols.size())
        return dd_set_error(DD_ERR_INVALID, "index out of range");
    auto &bt = r->batches[(size_t)b];
    memset(out, 0, sizeof(*out));
    out->data = bt.data[(size_t)c].data();
    out->data_len = (int64_t)bt.data[(size_t)c].size();
    out->validity = bt.validity[(size_t)c].empty() ? nullptr : bt.validity[(size_t)c].data();
    out->null_count = bt.null_count[(size_t)c];
    out->offsets = bt.offsets[(size_t)c].empty()
                       ? nullptr
                       : (const int32_t *)bt.offsets[(size_t)c].data();
    return DD_OK;
}
extern "C" void dd_ipc_reader_destroy(dd_ipc_reader *r) { delete r; }
