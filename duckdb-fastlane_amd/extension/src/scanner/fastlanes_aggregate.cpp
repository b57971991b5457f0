// fastlanes_aggregate.cpp -- `fastlanes_aggregate(path, aggregates[, filter])`.
//
// A table function that returns exactly one row: the ungrouped aggregates of
// one FastLanes file, reduced on the GPU under the filter (fls_aggregate), so
// only per-vector partial results cross PCIe instead of the qualifying rows.
//
//   aggregates: comma-separated `count(*)`, `count(c)`, `sum(c)`, `sum(a * b)`,
//               `min(c)`, `max(c)`, and `sum(F)`, `sum(F * F)`, `sum(F * F * F)`
//               over factors F: a column, `(literal - column)`,
//               `(literal + column)`, `(column + literal)` or
//               `(column - literal)`, the literal written as the filter writes
//               one for that column (TPC-H Q1's
//               `sum(l_extendedprice * (1 - l_discount) * (1 + l_tax))`); each
//               output column is named by the trimmed text of its item.
//               An item may end in `FILTER (WHERE <filter text>)` (keywords in
//               any case): the aggregate over the rows of the call's filter
//               where that condition holds too, in the grammar of the third
//               argument (IN lists, LIKE and column pairs included; no OR
//               group).  Items with identical condition text share
//               one condition (fls_aggregate_conditions, at most 8); the
//               item's name and type are what they are without the clause.
//   filter:     `term AND term ...`, a term `column op literal` (op one of
//               = != <> < <= > >=) or `column IS [NOT] NULL`.  Literals by
//               column type: integers, decimal numbers the column's scale
//               represents exactly, DATE 'YYYY-MM-DD', floats, single-quoted
//               strings ('' escapes a quote); IN lists, LIKE and column pairs
//               as table_function/filter_text.hpp describes them.  Among the
//               AND-ed items one parenthesised OR group may stand,
//                 filter := item (AND item)*
//                 item   := term | '(' branch (OR branch)+ ')'
//                 branch := term | '(' term (AND term)* ')'
//               with 2 to 8 branches (TPC-H Q19's shape): the branches become
//               the filter's alternatives (fls_scan_filter_alternatives).  No
//               OR outside parentheses, no second group, nothing nested deeper.
//
// `fastlanes_aggregate(path, aggregates, filter, group_by)` returns one row per
// group of a low-cardinality GROUP BY (fls_aggregate_grouped): group_by is a
// comma-separated list of 1 to 4 column names (integer-like, or dictionary-
// encoded VARCHAR), an empty or blank filter means none.  The key columns come
// first, named and typed as the table's, then the aggregates; rows are in
// order of each group's first row, in chunks of STANDARD_VECTOR_SIZE.  Past
// the engine's capacities (64 keys per 1024-row vector, 256 per row group) the
// query fails and the message points at read_fastlanes with a GROUP BY.
//
// Output types: counts and integer sums BIGINT, sums of DECIMAL(w, s)
// DECIMAL(18, s), sum(a * b) DECIMAL(18, s1 + s2) when an operand is DECIMAL,
// a sum of factors' product DECIMAL(18, sum of the scales) when a factor's
// column is DECIMAL (else BIGINT), float sums DOUBLE, min / max the column's
// own type.  The engine's sums are
// 128-bit; one that does not fit its output type raises OutOfRangeException
// (there is no HUGEINT here).  Everything unparsable, unknown or ill-typed is a
// BinderException quoting the offending text, raised at bind from the footer
// alone (no GPU).  DuckDB has no aggregate-pushdown hook for table functions:
// rewriting `SELECT sum(x) FROM read_fastlanes(...) WHERE ...` into this
// function would need an optimizer extension and is not attempted.
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>

#include "../../../../include/flsgpu.h"
#include "../../../../include/flswriter.h"
#include "../gpu_devices.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/common/string_util.hpp"
#include "duckdb/main/extension_util.hpp"
#include "table_function/fastlanes_aggregate.hpp"
#include "table_function/filter_text.hpp"
#include "type_mapping.hpp"

namespace duckdb {
namespace ext_fastlane {

namespace {

using namespace filter_text;  // the schema, lexer, literal and filter parsers shared with fastlanes_topn

struct AggTable {
    fls_table *table = nullptr;
    ~AggTable() {
        if (table) fls_table_close(table);
    }
};

struct AggBindData : public TableFunctionData {
    string file;
    std::vector<fls_aggregate_spec> specs;
    std::vector<fls_agg_expr> exprs;     // what the FLS_AGG_SUM_EXPR specs index (fls_aggregate_exprs)
    vector<LogicalType> types;
    vector<string> names;                // the items' trimmed text
    std::vector<fls_predicate> preds;
    std::deque<string> pred_strs;        // VARCHAR constants the predicates point at
    std::shared_ptr<KeySets> pred_sets = std::make_shared<KeySets>();  // the key sets of the filter's IN lists
    Alternatives alts;                   // the filter's OR group (fls_scan_filter_alternatives; empty: none)
    // the items' FILTER (WHERE ...) conditions: spec.cond - 1 indexes conds, which
    // index cond_preds (fls_aggregate_conditions); cond_texts[i] is condition i as written
    std::vector<fls_predicate> cond_preds;
    std::vector<fls_agg_condition> conds;
    vector<string> cond_texts;
    std::shared_ptr<AggTable> table;     // opened at bind (footer only)
    std::vector<uint32_t> keys;          // the group_by columns (empty: ungrouped, one row)
};

struct AggGlobalState : public GlobalTableFunctionState {
    std::mutex lock;
    bool done = false;
    fls_group_result *groups = nullptr;  // grouped: the result, emitted in chunks from `next`
    uint64_t next = 0;
    ~AggGlobalState() override {
        if (groups) fls_group_result_free(groups);
    }
};

int ColumnOf(const Schema &sch, const string &name, const string &item) {
    const string n = Trim(name);
    if (!(IsIdent(n) || (n.size() >= 2 && n.front() == '"' && n.back() == '"')))
        throw BinderException("fastlanes_aggregate: cannot parse \"" + n + "\" in aggregate \"" + item + "\"");
    const int c = sch.Find(n);
    if (c < 0) throw BinderException("fastlanes_aggregate: column \"" + n + "\" of aggregate \"" + item + "\" not found");
    return c;
}

// ---- the aggregate list ---------------------------------------------------
// One factor of a sum's product: a column, or a parenthesised column and
// literal joined by + or - (k + sign * column in the column's physical unit).
// `plain` tells a bare column.
fls_agg_factor ParseFactor(const Schema &sch, const string &text, const string &item, bool &plain) {
    fls_agg_factor f;
    memset(&f, 0, sizeof(f));
    f.sign = 1;
    auto check_type = [&](int c) {
        if (IsString(sch.cols[c].type) || IsFloat(sch.cols[c].type))
            throw BinderException("fastlanes_aggregate: sum of a product needs integer or DECIMAL columns, \"" +
                                  sch.names[c] + "\" is " + sch.types[c].ToString() + " in \"" + item + "\"");
    };
    plain = text.empty() || text.front() != '(';
    if (plain) {
        const int c = ColumnOf(sch, text, item);
        check_type(c);
        f.col = (uint32_t)c;
        return f;
    }
    const string inner = Trim(text.substr(1, text.size() - 2));
    // the operator: the first + or - past the first character (which may be the literal's sign)
    size_t op = string::npos;
    for (size_t i = 1; i < inner.size() && op == string::npos; ++i)
        if (inner[i] == '+' || inner[i] == '-') op = i;
    if (op == string::npos)
        throw BinderException("fastlanes_aggregate: cannot parse factor \"" + text + "\" in aggregate \"" + item + "\"");
    const string lhs = Trim(inner.substr(0, op)), rhs = Trim(inner.substr(op + 1));
    auto is_col = [&](const string &n) {
        return (IsIdent(n) || (n.size() >= 2 && n.front() == '"' && n.back() == '"')) && sch.Find(n) >= 0;
    };
    const bool lcol = is_col(lhs), rcol = is_col(rhs);
    if (lcol == rcol)
        throw BinderException(string("fastlanes_aggregate: a factor needs one column and one literal, \"") + text +
                              "\" has " + (lcol ? "two columns" : "no column") + " in aggregate \"" + item + "\"");
    const int c = sch.Find(lcol ? lhs : rhs);
    check_type(c);
    f.col = (uint32_t)c;
    const string lit = lcol ? rhs : lhs;
    if (lit.empty())
        throw BinderException("fastlanes_aggregate: cannot parse factor \"" + text + "\" in aggregate \"" + item + "\"");
    fls_predicate p;
    memset(&p, 0, sizeof(p));
    std::deque<string> strs;
    Lexer lex(lit);
    SetLiteral(sch, c, lex, lex.Next(), item, p, strs, "aggregate");
    if (lex.Next().kind != Token::END)
        throw BinderException("fastlanes_aggregate: cannot parse \"" + lit + "\" in aggregate \"" + item + "\"");
    const bool is_unsigned = sch.cols[c].type >= FLS_UINT8 && sch.cols[c].type <= FLS_UINT64;
    const bool minus = inner[op] == '-';
    // k is an int64: an unsigned literal past it, or the negation of the lowest one, has no place
    if ((is_unsigned && p.value > (uint64_t)INT64_MAX) || (lcol && minus && p.value == (1ull << 63)))
        throw BinderException("fastlanes_aggregate: \"" + lit + "\" is not in range for a factor of aggregate \"" + item +
                              "\"");
    f.k = (int64_t)p.value;
    if (lcol && minus) f.k = -f.k;       // (column - literal)
    if (!lcol && minus) f.sign = -1;     // (literal - column)
    return f;
}

// one item of the aggregate list -> spec and output type; a sum of factors
// that is not a plain column or the product of two appends its expression
void ParseAggregate(const Schema &sch, const string &item, fls_aggregate_spec &spec, LogicalType &type,
                    std::vector<fls_agg_expr> &exprs) {
    memset(&spec, 0, sizeof(spec));
    const size_t open = item.find('(');
    if (open == string::npos || item.back() != ')')
        throw BinderException("fastlanes_aggregate: cannot parse aggregate \"" + item + "\"");
    const string fn = StringUtil::Lower(Trim(item.substr(0, open)));
    const string arg = Trim(item.substr(open + 1, item.size() - open - 2));
    if (arg.empty() || (fn != "sum" && (arg.find('(') != string::npos || arg.find(')') != string::npos)))
        throw BinderException("fastlanes_aggregate: cannot parse aggregate \"" + item + "\"");
    if (fn == "count") {
        type = LogicalType::BIGINT;
        if (arg == "*") {
            spec.fn = FLS_AGG_COUNT_STAR;
            return;
        }
        spec.fn = FLS_AGG_COUNT;
        spec.col = (uint32_t)ColumnOf(sch, arg, item);
        return;
    }
    if (fn != "sum" && fn != "min" && fn != "max")
        throw BinderException("fastlanes_aggregate: unknown aggregate function \"" + fn + "\" in \"" + item + "\"");
    // the factors: split at * outside parentheses, which do not nest
    std::vector<string> parts;
    {
        int depth = 0;
        size_t start = 0;
        for (size_t i = 0; i <= arg.size(); ++i) {
            if (i < arg.size() && arg[i] == '(') ++depth;
            if (i < arg.size() && arg[i] == ')') --depth;
            if (depth < 0 || depth > 1)
                throw BinderException("fastlanes_aggregate: unbalanced or nested parentheses in aggregate \"" + item + "\"");
            if (i == arg.size() || (arg[i] == '*' && depth == 0)) {
                parts.push_back(Trim(arg.substr(start, i - start)));
                start = i + 1;
            }
        }
        if (depth != 0)
            throw BinderException("fastlanes_aggregate: unbalanced or nested parentheses in aggregate \"" + item + "\"");
    }
    const bool parens = arg.find('(') != string::npos;
    if (parts.size() > 1 || parens) {
        if (fn != "sum") throw BinderException("fastlanes_aggregate: a product is only supported in sum(): \"" + item + "\"");
        if (parts.size() > 3)
            throw BinderException("fastlanes_aggregate: at most 3 factors in a product, \"" + item + "\" holds " +
                                  std::to_string(parts.size()));
        fls_agg_expr e;
        memset(&e, 0, sizeof(e));
        bool all_plain = true, dec = false;
        unsigned scale = 0;
        for (const string &part : parts) {
            if (part.size() >= 2 && part.front() == '(' && part.back() != ')')
                throw BinderException("fastlanes_aggregate: cannot parse factor \"" + part + "\" in aggregate \"" + item +
                                      "\"");
            bool plain;
            const fls_agg_factor f = ParseFactor(sch, part, item, plain);
            all_plain = all_plain && plain;
            e.f[e.nfactors++] = f;
            if (sch.cols[f.col].type == FLS_DECIMAL) {
                dec = true;
                scale += sch.cols[f.col].scale;
            }
        }
        if (scale > 18)
            throw BinderException("fastlanes_aggregate: the scale of \"" + item + "\" exceeds DECIMAL(18)");
        type = dec ? LogicalType::DECIMAL(18, (uint8_t)scale) : LogicalType::BIGINT;
        if (all_plain && e.nfactors == 2) {  // the product of two columns
            spec.fn = FLS_AGG_SUM_PRODUCT;
            spec.col = e.f[0].col;
            spec.col2 = e.f[1].col;
            return;
        }
        spec.fn = FLS_AGG_SUM_EXPR;
        spec.col = (uint32_t)exprs.size();
        exprs.push_back(e);
        return;
    }
    const int c = ColumnOf(sch, arg, item);
    if (IsString(sch.cols[c].type))
        throw BinderException("fastlanes_aggregate: " + fn + " of " + sch.types[c].ToString() + " column \"" + sch.names[c] +
                              "\" is not supported in \"" + item + "\"");
    spec.col = (uint32_t)c;
    if (fn == "sum") {
        spec.fn = FLS_AGG_SUM;
        type = IsFloat(sch.cols[c].type)           ? LogicalType::DOUBLE
               : sch.cols[c].type == FLS_DECIMAL ? LogicalType::DECIMAL(18, sch.cols[c].scale)
                                                 : LogicalType::BIGINT;
    } else {
        spec.fn = fn == "min" ? FLS_AGG_MIN : FLS_AGG_MAX;
        type = sch.types[c];
    }
}

// An item's trailing `FILTER (WHERE text)`: the aggregate before it into agg,
// the condition's text into cond; false when the item has no such clause.
bool SplitFilterClause(const string &item, string &agg, string &cond) {
    agg = item;
    // the aggregate ends at the parenthesis that closes its first one (its literals hold none)
    size_t close = string::npos;
    int depth = 0;
    for (size_t i = 0; i < item.size() && close == string::npos; ++i) {
        if (item[i] == '(') ++depth;
        if (item[i] == ')' && --depth == 0) close = i;
    }
    if (close == string::npos || close + 1 == item.size()) return false;
    const string rest = Trim(item.substr(close + 1));
    if (rest.empty()) return false;
    auto bad = [&]() {
        return BinderException("fastlanes_aggregate: FILTER (WHERE ...) is expected after the aggregate at \"" + rest +
                               "\" in \"" + item + "\"");
    };
    if (rest.size() < 6 || StringUtil::Lower(rest.substr(0, 6)) != "filter") throw bad();
    const string paren = Trim(rest.substr(6));
    if (paren.size() < 2 || paren.front() != '(' || paren.back() != ')') throw bad();
    const string inner = Trim(paren.substr(1, paren.size() - 2));
    if (inner.size() < 6 || StringUtil::Lower(inner.substr(0, 5)) != "where" || !isspace((unsigned char)inner[5])) throw bad();
    cond = Trim(inner.substr(5));
    if (cond.empty()) throw bad();
    agg = item.substr(0, close + 1);
    return true;
}

// the group_by text: 1 to 4 column names separated by commas
void ParseGroupBy(const Schema &sch, const string &list, std::vector<uint32_t> &keys, vector<string> &names,
                  vector<LogicalType> &types) {
    size_t start = 0;
    for (size_t i = 0; i <= list.size(); ++i) {
        if (i < list.size() && list[i] != ',') continue;
        const string item = Trim(list.substr(start, i - start));
        start = i + 1;
        if (item.empty()) throw BinderException("fastlanes_aggregate: empty item in group_by list \"" + list + "\"");
        const int c = sch.Find(item);
        if (c < 0)
            throw BinderException("fastlanes_aggregate: column \"" + item + "\" of group_by \"" + list + "\" not found");
        const uint8_t ty = sch.cols[c].type;
        if (IsFloat(ty) || ty == FLS_BLOB)
            throw BinderException("fastlanes_aggregate: group_by key \"" + item + "\" is " + sch.types[c].ToString() +
                                  ": FLOAT, DOUBLE and BLOB columns cannot be keys, in \"" + list + "\"");
        for (uint32_t k : keys)
            if (k == (uint32_t)c)
                throw BinderException("fastlanes_aggregate: group_by key \"" + item + "\" is listed twice in \"" + list + "\"");
        keys.push_back((uint32_t)c);
        names.push_back(sch.names[c]);
        types.push_back(sch.types[c]);
    }
    if (keys.size() > 4)
        throw BinderException("fastlanes_aggregate: at most 4 group_by keys, \"" + list + "\" holds " +
                              std::to_string(keys.size()));
}

unique_ptr<FunctionData> AggBind(ClientContext &, TableFunctionBindInput &input, vector<LogicalType> &return_types,
                                 vector<string> &names) {
    if (input.inputs.size() < 2 || input.inputs.size() > 4)
        throw BinderException("fastlanes_aggregate takes (path, aggregates[, filter[, group_by]])");
    for (auto &v : input.inputs)
        if (v.IsNull() || v.type() != LogicalType::VARCHAR)
            throw BinderException("fastlanes_aggregate arguments must be strings");
    auto bind = make_uniq<AggBindData>();
    bind->file = input.inputs[0].GetValue<string>();
    bind->table = std::make_shared<AggTable>();
    fls_connection *conn = SharedConnection();
    if (!conn || fls_read_fls(conn, bind->file.c_str(), &bind->table->table) != 0)
        throw BinderException("Failed to open FastLanes file: " + bind->file);
    Schema sch;
    sch.Load(bind->table->table);
    // the aggregate list: items separated by commas outside parentheses and
    // outside the quoted strings of a FILTER clause
    const string list = input.inputs[1].GetValue<string>();
    vector<string> items;
    int depth = 0;
    bool quoted = false;
    size_t start = 0;
    for (size_t i = 0; i <= list.size(); ++i) {
        if (i < list.size() && list[i] == '\'') quoted = !quoted;
        if (i < list.size() && quoted) continue;
        if (i < list.size() && list[i] == '(') ++depth;
        if (i < list.size() && list[i] == ')') --depth;
        if (i == list.size() || (list[i] == ',' && depth == 0)) {
            items.push_back(Trim(list.substr(start, i - start)));
            start = i + 1;
        }
    }
    for (auto &item : items) {
        if (item.empty()) throw BinderException("fastlanes_aggregate: empty item in aggregate list \"" + list + "\"");
        fls_aggregate_spec spec;
        LogicalType type;
        string agg, cond;
        const bool conditioned = SplitFilterClause(item, agg, cond);
        ParseAggregate(sch, agg, spec, type, bind->exprs);
        if (conditioned) {
            size_t k = 0;
            while (k < bind->cond_texts.size() && bind->cond_texts[k] != cond) ++k;
            if (k == bind->cond_texts.size()) {
                if (k == 8)
                    throw BinderException("fastlanes_aggregate: at most 8 different FILTER conditions per call, \"" + cond +
                                          "\" of \"" + item + "\" is the 9th");
                fls_agg_condition c;
                c.first = (uint32_t)bind->cond_preds.size();
                ParseFilter(sch, cond, bind->cond_preds, bind->pred_strs, "fastlanes_aggregate", conn, bind->pred_sets.get());
                c.n = (uint32_t)bind->cond_preds.size() - c.first;
                bind->conds.push_back(c);
                bind->cond_texts.push_back(cond);
            }
            spec.cond = (uint32_t)k + 1;
        }
        bind->specs.push_back(spec);
        bind->types.push_back(type);
        names.push_back(item);
        bind->names.push_back(item);
    }
    if (bind->specs.size() > 32)
        throw BinderException("fastlanes_aggregate: at most 32 aggregates per call, \"" + list + "\" holds " +
                              std::to_string(bind->specs.size()));
    if (input.inputs.size() >= 3)
        ParseFilter(sch, input.inputs[2].GetValue<string>(), bind->preds, bind->pred_strs, "fastlanes_aggregate", conn,
                    bind->pred_sets.get(), &bind->alts);
    return_types = bind->types;
    if (input.inputs.size() == 4) {
        // the key columns come first, named and typed as the table's columns
        vector<string> key_names;
        vector<LogicalType> key_types;
        ParseGroupBy(sch, input.inputs[3].GetValue<string>(), bind->keys, key_names, key_types);
        names.insert(names.begin(), key_names.begin(), key_names.end());
        return_types.insert(return_types.begin(), key_types.begin(), key_types.end());
    }
    return std::move(bind);
}

unique_ptr<GlobalTableFunctionState> AggInitGlobal(ClientContext &, TableFunctionInitInput &) {
    return make_uniq<AggGlobalState>();
}

// the 128-bit value as an int64, or OutOfRangeException
int64_t Narrow(const fls_aggregate_value &v, const string &name, const LogicalType &type) {
    const bool fits = v.hi == ((v.lo >> 63) ? ~0ull : 0ull);
    const int64_t x = (int64_t)v.lo;
    const bool dec_ok = type.id() != LogicalTypeId::DECIMAL || (x > -1000000000000000000ll && x < 1000000000000000000ll);
    if (!fits || !dec_ok)
        throw OutOfRangeException("fastlanes_aggregate: " + name + " does not fit " + type.ToString() +
                                  " (the 128-bit sum is available through fls_aggregate)");
    return x;
}

// one aggregate value into row `row` of its output column
void EmitValue(const AggBindData &bind, idx_t j, const fls_aggregate_value &v, Vector &vec, idx_t row) {
    if (v.kind == FLS_AGGV_NULL) {
        vec.SetValue(row, Value());
    } else if (v.kind == FLS_AGGV_DOUBLE) {
        double d;
        memcpy(&d, &v.lo, 8);
        vec.SetValue(row, Value::DOUBLE(d));
    } else if (bind.specs[j].fn == FLS_AGG_MIN || bind.specs[j].fn == FLS_AGG_MAX) {
        vec.SetValue(row, Value::BIGINT((int64_t)v.lo));  // the column's own type: its low bytes
    } else {
        vec.SetValue(row, Value::BIGINT(Narrow(v, bind.names[j], bind.types[j])));
    }
}

// The grouped form: the first call runs fls_aggregate_grouped, every call
// emits the next STANDARD_VECTOR_SIZE groups at most, in the C call's order.
void AggScanGrouped(const AggBindData &bind, AggGlobalState &g, DataChunk &output) {
    std::lock_guard<std::mutex> guard(g.lock);
    fls_table *t = bind.table->table;
    if (!g.done) {
        g.done = true;
        if (fls_scan_filter(t, bind.preds.data(), (uint32_t)bind.preds.size()) != 0 ||
            fls_scan_filter_alternatives(t, bind.alts.preds.data(), (uint32_t)bind.alts.preds.size(),
                                         bind.alts.ranges.data(), (uint32_t)bind.alts.ranges.size()) != 0 ||
            fls_aggregate_exprs(t, bind.exprs.data(), (uint32_t)bind.exprs.size()) != 0 ||
            fls_aggregate_conditions(t, bind.cond_preds.data(), (uint32_t)bind.cond_preds.size(), bind.conds.data(),
                                     (uint32_t)bind.conds.size()) != 0)
            throw IOException(string("FastLanes aggregate failed: ") + fls_last_error());
        const int rc = fls_aggregate_grouped(t, bind.keys.data(), (uint32_t)bind.keys.size(), bind.specs.data(),
                                             (uint32_t)bind.specs.size(), 0, fls_table_nrowgroups(t), &g.groups);
        const string err = rc ? fls_last_error() : "";
        fls_scan_filter(t, nullptr, 0);
        fls_scan_filter_alternatives(t, nullptr, 0, nullptr, 0);
        fls_aggregate_exprs(t, nullptr, 0);
        fls_aggregate_conditions(t, nullptr, 0, nullptr, 0);
        if (rc == FLS_ERR_LIMIT)
            throw InvalidInputException("fastlanes_aggregate: " + err +
                                        "; use SELECT ... FROM read_fastlanes(...) GROUP BY ... instead");
        if (rc == FLS_ERR_ARG) throw InvalidInputException("fastlanes_aggregate: " + err);  // a key's chunks, the SUM_PRODUCT bound
        if (rc) throw IOException("FastLanes aggregate failed: " + err);
    }
    const uint64_t total = fls_group_result_ngroups(g.groups);
    const idx_t nk = bind.keys.size();
    idx_t n = 0;
    for (; n < STANDARD_VECTOR_SIZE && g.next < total; ++n, ++g.next) {
        for (idx_t q = 0; q < nk; ++q) {
            fls_group_key k;
            if (fls_group_result_key(g.groups, g.next, (uint32_t)q, &k) != 0)
                throw IOException(string("FastLanes aggregate failed: ") + fls_last_error());
            Vector &vec = output.data[q];
            if (k.kind == FLS_KEYV_NULL) vec.SetValue(n, Value());
            else if (k.kind == FLS_KEYV_STRING) vec.SetValue(n, Value(string(k.str ? k.str : "", (size_t)k.str_len)));
            else vec.SetValue(n, Value::BIGINT((int64_t)k.lo));  // the column's own type: its low bytes
        }
        const fls_aggregate_value *vals = fls_group_result_values(g.groups, g.next);
        for (idx_t j = 0; j < bind.specs.size() && nk + j < output.ColumnCount(); ++j)
            EmitValue(bind, j, vals[j], output.data[nk + j], n);
    }
    output.SetCardinality(n);
}

void AggScan(ClientContext &, TableFunctionInput &data, DataChunk &output) {
    const auto &bind = data.bind_data->Cast<AggBindData>();
    auto &g = data.global_state->Cast<AggGlobalState>();
    output.Reset();
    if (!bind.keys.empty()) {
        AggScanGrouped(bind, g, output);
        return;
    }
    {
        std::lock_guard<std::mutex> guard(g.lock);
        if (g.done) {
            output.SetCardinality(0);
            return;
        }
        g.done = true;
    }
    fls_table *t = bind.table->table;
    std::vector<fls_aggregate_value> vals(bind.specs.size());
    if (fls_scan_filter(t, bind.preds.data(), (uint32_t)bind.preds.size()) != 0 ||
        fls_scan_filter_alternatives(t, bind.alts.preds.data(), (uint32_t)bind.alts.preds.size(), bind.alts.ranges.data(),
                                     (uint32_t)bind.alts.ranges.size()) != 0 ||
        fls_aggregate_exprs(t, bind.exprs.data(), (uint32_t)bind.exprs.size()) != 0 ||
        fls_aggregate_conditions(t, bind.cond_preds.data(), (uint32_t)bind.cond_preds.size(), bind.conds.data(),
                                 (uint32_t)bind.conds.size()) != 0)
        throw IOException(string("FastLanes aggregate failed: ") + fls_last_error());
    const int rc = fls_aggregate(t, bind.specs.data(), (uint32_t)bind.specs.size(), 0, fls_table_nrowgroups(t), vals.data());
    const string err = rc ? fls_last_error() : "";
    fls_scan_filter(t, nullptr, 0);
    fls_scan_filter_alternatives(t, nullptr, 0, nullptr, 0);
    fls_aggregate_exprs(t, nullptr, 0);
    fls_aggregate_conditions(t, nullptr, 0, nullptr, 0);
    if (rc == FLS_ERR_ARG) throw OutOfRangeException("fastlanes_aggregate: " + err);  // the SUM_PRODUCT / SUM_EXPR bound
    if (rc) throw IOException("FastLanes aggregate failed: " + err);
    for (idx_t j = 0; j < output.ColumnCount() && j < vals.size(); ++j) EmitValue(bind, j, vals[j], output.data[j], 0);
    output.SetCardinality(1);
}

}  // namespace

void RegisterFastlanesAggregate(DatabaseInstance &db) {
    TableFunction fn("fastlanes_aggregate", {LogicalType::VARCHAR, LogicalType::VARCHAR}, AggScan, AggBind, AggInitGlobal);
    ExtensionUtil::RegisterFunction(db, fn);
    fn.arguments = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR};
    ExtensionUtil::RegisterFunction(db, fn);
    fn.arguments = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR};
    ExtensionUtil::RegisterFunction(db, fn);
}

}  // namespace ext_fastlane
}  // namespace duckdb
