// fastlanes_topn.cpp -- `fastlanes_topn(path, order_by, k[, filter[, columns]])`.
//
// A table function that returns the k best rows of one FastLanes file ordered
// by one column, selected on the GPU under the filter (fls_topn): per row
// group a list of at most k 16-byte candidates crosses PCIe instead of the
// qualifying rows, and only the winners' row groups are decoded for the
// delivered columns.
//
//   order_by: `column [ASC | DESC] [NULLS FIRST | NULLS LAST]`; the column is
//             matched as fastlanes_aggregate matches identifiers.  ASC and
//             NULLS LAST are the defaults (DuckDB's).  Integer-like, DATE,
//             DECIMAL, FLOAT and DOUBLE columns; equal keys come in table
//             order.
//   k:        INTEGER, 0 to 1024.
//   filter:   fastlanes_aggregate's grammar (table_function/filter_text.hpp),
//             its one parenthesised OR group included:
//               filter := item (AND item)*
//               item   := term | '(' branch (OR branch)+ ')'
//               branch := term | '(' term (AND term)* ')'
//             empty or blank means none.
//   columns:  a comma-separated list of the columns to return, in that
//             order; empty or absent means all, in table order.
//
// The output columns are named and typed as read_fastlanes types them; rows
// come in result order, in chunks of STANDARD_VECTOR_SIZE.  Everything
// unparsable, unknown or ill-typed is a BinderException quoting the offending
// text, raised at bind from the footer alone (no GPU).  Rewriting `SELECT ...
// FROM read_fastlanes(...) ORDER BY c LIMIT k` into this function would need
// an optimizer extension and is not attempted.
#include <cstring>
#include <memory>
#include <mutex>

#include "../gpu_devices.hpp"
#include "duckdb/main/extension_util.hpp"
#include "table_function/fastlanes_topn.hpp"
#include "table_function/filter_text.hpp"

namespace duckdb {
namespace ext_fastlane {

namespace {

using namespace filter_text;

constexpr const char *kWho = "fastlanes_topn";
constexpr int32_t kMaxK = 1024;  // fls_topn's cap (kMaxTopN)

struct TopnTable {
    fls_table *table = nullptr;
    ~TopnTable() {
        if (table) fls_table_close(table);
    }
};

struct TopnBindData : public TableFunctionData {
    string file;
    fls_order_key key;
    uint32_t k = 0;
    std::vector<uint32_t> out_cols;      // table columns returned, in output order
    std::vector<fls_column_info> infos;  // ... and their types
    std::vector<uint8_t> mask;           // fls_topn's col_mask
    std::vector<fls_predicate> preds;
    std::deque<string> pred_strs;        // VARCHAR constants the predicates point at
    std::shared_ptr<KeySets> pred_sets = std::make_shared<KeySets>();  // the key sets of the filter's IN lists
    Alternatives alts;                   // the filter's OR group (fls_scan_filter_alternatives; empty: none)
    std::shared_ptr<TopnTable> table;    // opened at bind (footer only)
};

struct TopnGlobalState : public GlobalTableFunctionState {
    std::mutex lock;
    bool done = false;
    fls_topn_result *result = nullptr;   // emitted in chunks from `next`
    uint64_t next = 0;
    ~TopnGlobalState() override {
        if (result) fls_topn_result_free(result);
    }
};

// `column [ASC | DESC] [NULLS FIRST | NULLS LAST]`
void ParseOrderBy(const Schema &sch, const string &text, fls_order_key &key) {
    auto malformed = [&](const string &at) {
        return BinderException(string(kWho) + ": cannot parse \"" + at + "\" in order_by \"" + text +
                               "\" (column [ASC | DESC] [NULLS FIRST | NULLS LAST])");
    };
    const string s = Trim(text);
    if (s.empty()) throw malformed("");
    // the column: a quoted identifier (which may hold blanks) or a word
    size_t end;
    if (s[0] == '"') {
        end = s.find('"', 1);
        if (end == string::npos) throw malformed(s);
        ++end;
    } else {
        end = 0;
        while (end < s.size() && !isspace((unsigned char)s[end])) ++end;
    }
    const string col = s.substr(0, end);
    if (!(IsIdent(col) || col[0] == '"')) throw malformed(col);
    if (end < s.size() && !isspace((unsigned char)s[end])) throw malformed(s.substr(end));
    const int c = sch.Find(col);
    if (c < 0) throw BinderException(string(kWho) + ": column \"" + col + "\" of order_by \"" + text + "\" not found");
    if (IsString(sch.cols[c].type))
        throw BinderException(string(kWho) + ": order_by column \"" + sch.names[c] + "\" is " + sch.types[c].ToString() +
                              ": VARCHAR and BLOB columns cannot be ordered by, in \"" + text + "\"");
    memset(&key, 0, sizeof(key));
    key.col = (uint32_t)c;
    vector<string> words;
    for (size_t i = end; i < s.size();) {
        while (i < s.size() && isspace((unsigned char)s[i])) ++i;
        size_t j = i;
        while (j < s.size() && !isspace((unsigned char)s[j])) ++j;
        if (j > i) words.push_back(StringUtil::Lower(s.substr(i, j - i)));
        i = j;
    }
    size_t w = 0;
    if (w < words.size() && (words[w] == "asc" || words[w] == "desc")) key.desc = words[w++] == "desc";
    if (w < words.size() && words[w] == "nulls") {
        if (w + 1 >= words.size() || (words[w + 1] != "first" && words[w + 1] != "last"))
            throw malformed(w + 1 < words.size() ? words[w] + " " + words[w + 1] : words[w]);
        key.nulls_first = words[w + 1] == "first";
        w += 2;
    }
    if (w < words.size()) throw malformed(words[w]);
}

// the columns text: names separated by commas; blank = every column in table order
void ParseColumns(const Schema &sch, const string &list, std::vector<uint32_t> &cols) {
    if (Trim(list).empty()) {
        for (uint32_t c = 0; c < sch.cols.size(); ++c) cols.push_back(c);
        return;
    }
    size_t start = 0;
    for (size_t i = 0; i <= list.size(); ++i) {
        if (i < list.size() && list[i] != ',') continue;
        const string item = Trim(list.substr(start, i - start));
        start = i + 1;
        if (item.empty()) throw BinderException(string(kWho) + ": empty item in columns list \"" + list + "\"");
        const int c = sch.Find(item);
        if (c < 0) throw BinderException(string(kWho) + ": column \"" + item + "\" of columns \"" + list + "\" not found");
        for (uint32_t o : cols)
            if (o == (uint32_t)c)
                throw BinderException(string(kWho) + ": column \"" + item + "\" is listed twice in columns \"" + list + "\"");
        cols.push_back((uint32_t)c);
    }
}

unique_ptr<FunctionData> TopnBind(ClientContext &, TableFunctionBindInput &input, vector<LogicalType> &return_types,
                                  vector<string> &names) {
    if (input.inputs.size() < 3 || input.inputs.size() > 5)
        throw BinderException("fastlanes_topn takes (path, order_by, k[, filter[, columns]])");
    for (size_t i = 0; i < input.inputs.size(); ++i) {
        if (i == 2) continue;
        if (input.inputs[i].IsNull() || input.inputs[i].type() != LogicalType::VARCHAR)
            throw BinderException("fastlanes_topn arguments must be strings, except k");
    }
    if (input.inputs[2].IsNull() || input.inputs[2].type() != LogicalType::INTEGER)
        throw BinderException("fastlanes_topn: k must be an INTEGER");
    const int32_t k = input.inputs[2].GetValue<int32_t>();
    if (k < 0) throw BinderException(string(kWho) + ": k must not be negative, got \"" + std::to_string(k) + "\"");
    if (k > kMaxK)
        throw InvalidInputException(string(kWho) + ": k = " + std::to_string(k) + " is above the limit of " +
                                    std::to_string(kMaxK) + " rows; use SELECT ... FROM read_fastlanes(...) ORDER BY ... "
                                    "LIMIT " + std::to_string(k) + " instead");
    auto bind = make_uniq<TopnBindData>();
    bind->file = input.inputs[0].GetValue<string>();
    bind->k = (uint32_t)k;
    bind->table = std::make_shared<TopnTable>();
    fls_connection *conn = SharedConnection();
    if (!conn || fls_read_fls(conn, bind->file.c_str(), &bind->table->table) != 0)
        throw BinderException("Failed to open FastLanes file: " + bind->file);
    Schema sch;
    sch.Load(bind->table->table);
    ParseOrderBy(sch, input.inputs[1].GetValue<string>(), bind->key);
    if (input.inputs.size() >= 4)
        ParseFilter(sch, input.inputs[3].GetValue<string>(), bind->preds, bind->pred_strs, kWho, conn,
                    bind->pred_sets.get(), &bind->alts);
    ParseColumns(sch, input.inputs.size() == 5 ? input.inputs[4].GetValue<string>() : string(), bind->out_cols);
    bind->mask.assign(sch.cols.size(), 0);
    for (uint32_t c : bind->out_cols) {
        bind->mask[c] = 1;
        bind->infos.push_back(sch.cols[c]);
        names.push_back(sch.names[c]);
        return_types.push_back(sch.types[c]);
    }
    return std::move(bind);
}

unique_ptr<GlobalTableFunctionState> TopnInitGlobal(ClientContext &, TableFunctionInitInput &) {
    return make_uniq<TopnGlobalState>();
}

// the value at p (the scan's physical layout) as a Value of the column's type
Value ValueAt(const fls_column_info &ci, const uint8_t *p) {
    auto ld = [p](auto x) {
        memcpy(&x, p, sizeof(x));
        return x;
    };
    switch (ci.type) {
    case FLS_INT8: return Value::TINYINT(ld(int8_t()));
    case FLS_INT16: return Value::SMALLINT(ld(int16_t()));
    case FLS_INT32: return Value::INTEGER(ld(int32_t()));
    case FLS_INT64: return Value::BIGINT(ld(int64_t()));
    case FLS_UINT8: return Value::UTINYINT(ld(uint8_t()));
    case FLS_UINT16: return Value::USMALLINT(ld(uint16_t()));
    case FLS_UINT32: return Value::UINTEGER(ld(uint32_t()));
    case FLS_UINT64: return Value::UBIGINT(ld(uint64_t()));
    case FLS_BOOLEAN: return Value::BOOLEAN(ld(uint8_t()) != 0);
    case FLS_DATE: return Value::DATE(date_t{ld(int32_t())});
    case FLS_DECIMAL: return Value::DECIMAL(ld(int64_t()), ci.width, ci.scale);
    case FLS_FLOAT: return Value::FLOAT(ld(float()));
    case FLS_DOUBLE: return Value::DOUBLE(ld(double()));
    default: break;
    }
    // VARCHAR / BLOB: a 16-byte string_t record, long strings through its pointer
    const uint32_t len = ld(uint32_t());
    const uint8_t *bytes = p + 4;
    if (len > 12) memcpy(&bytes, p + 8, 8);
    if (ci.type == FLS_BLOB) return Value::BLOB(bytes, len);
    return Value(string((const char *)bytes, len));
}

// The first call runs fls_topn; every call emits the next STANDARD_VECTOR_SIZE
// rows at most, in result order.
void TopnScan(ClientContext &, TableFunctionInput &data, DataChunk &output) {
    const auto &bind = data.bind_data->Cast<TopnBindData>();
    auto &g = data.global_state->Cast<TopnGlobalState>();
    output.Reset();
    std::lock_guard<std::mutex> guard(g.lock);
    fls_table *t = bind.table->table;
    if (!g.done) {
        g.done = true;
        if (fls_scan_filter(t, bind.preds.data(), (uint32_t)bind.preds.size()) != 0 ||
            fls_scan_filter_alternatives(t, bind.alts.preds.data(), (uint32_t)bind.alts.preds.size(),
                                         bind.alts.ranges.data(), (uint32_t)bind.alts.ranges.size()) != 0)
            throw IOException(string("FastLanes top-N failed: ") + fls_last_error());
        const int rc = fls_topn(t, &bind.key, bind.k, bind.mask.data(), 0, fls_table_nrowgroups(t), &g.result);
        const string err = rc ? fls_last_error() : "";
        fls_scan_filter(t, nullptr, 0);
        fls_scan_filter_alternatives(t, nullptr, 0, nullptr, 0);
        if (rc == FLS_ERR_ARG || rc == FLS_ERR_LIMIT) throw InvalidInputException(string(kWho) + ": " + err);
        if (rc) throw IOException("FastLanes top-N failed: " + err);
    }
    const uint64_t total = fls_topn_result_nrows(g.result);
    const idx_t n = (idx_t)std::min<uint64_t>(STANDARD_VECTOR_SIZE, total - g.next);
    for (idx_t j = 0; j < bind.out_cols.size() && j < output.ColumnCount() && n > 0; ++j) {
        const void *values = nullptr;
        const uint64_t *validity = nullptr;
        if (fls_topn_result_column(g.result, bind.out_cols[j], &values, &validity) != 0)
            throw IOException(string("FastLanes top-N failed: ") + fls_last_error());
        const fls_column_info &ci = bind.infos[j];
        Vector &vec = output.data[j];
        for (idx_t i = 0; i < n; ++i) {
            const uint64_t row = g.next + i;
            if (validity && !((validity[row >> 6] >> (row & 63)) & 1)) vec.SetValue(i, Value());
            else vec.SetValue(i, ValueAt(ci, (const uint8_t *)values + row * ci.out_bytes));
        }
    }
    g.next += n;
    output.SetCardinality(n);
}

}  // namespace

void RegisterFastlanesTopn(DatabaseInstance &db) {
    TableFunction fn("fastlanes_topn", {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::INTEGER}, TopnScan,
                     TopnBind, TopnInitGlobal);
    ExtensionUtil::RegisterFunction(db, fn);
    fn.arguments = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::INTEGER, LogicalType::VARCHAR};
    ExtensionUtil::RegisterFunction(db, fn);
    fn.arguments = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::INTEGER, LogicalType::VARCHAR,
                    LogicalType::VARCHAR};
    ExtensionUtil::RegisterFunction(db, fn);
}

}  // namespace ext_fastlane
}  // namespace duckdb
