//===----------------------------------------------------------------------===//
//                         DuckDB - fastlane (MI355X)
//
// table_function/filter_text.hpp -- the text grammar the pushdown table
// functions share (`fastlanes_aggregate`, `fastlanes_topn`): the table's
// schema with DuckDB's identifier matching, the lexer, the literal parser by
// column type and the filter `term AND term ...` -> fls_predicate[].
//
//   filter: a term is `column op literal` (op one of = != <> < <= > >=) or
//           `column IS [NOT] NULL`.  Literals by column type: integers,
//           decimal numbers the column's scale represents exactly,
//           DATE 'YYYY-MM-DD', floats, single-quoted strings ('' escapes a
//           quote).  `column [NOT] IN (literal, ...)` is a term too: on an
//           integer-like column the list becomes one key-set term
//           (fls_keyset_create, FLS_CMP_IN_SET / FLS_CMP_NOT_IN_SET), on
//           VARCHAR / FLOAT / DOUBLE EQ terms of one clause (NOT IN: NE terms,
//           a clause each); NULL in the list follows SQL.
//           `column [NOT] LIKE 'pattern' [ESCAPE 'c']` on a VARCHAR column is
//           one pattern term (FLS_CMP_LIKE / FLS_CMP_NOT_LIKE: `%` any bytes,
//           `_` one character, case-sensitive; c one byte; LIKE NULL matches
//           no row).  `column op column` compares two columns of the same
//           row (FLS_CMP_COL_EQ .. FLS_CMP_COL_GE): the right side is a
//           column when it is an identifier the schema resolves and neither
//           NULL nor the start of a typed literal (DATE '...'); a word that
//           names no column is read as a literal as before (nan, inf, true).
//
//   filter := item (AND item)*
//   item   := term | '(' branch (OR branch)+ ')'
//   branch := term | '(' term (AND term)* ')'
//           One parenthesised OR group (2 to 8 branches) may stand among the
//           AND-ed items: its branches become the filter's alternatives
//           (fls_scan_filter_alternatives), a row passing when the AND-ed terms
//           hold and at least one branch does.  No OR outside parentheses, no
//           second group, no parenthesis inside a branch's own, no group in an
//           aggregate's FILTER (WHERE ...) condition.
//
// Everything unparsable, unknown or ill-typed is a BinderException that starts
// with the calling function's name (`who`) and quotes the offending text.
//===----------------------------------------------------------------------===//
#pragma once

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "../../../../../include/flsgpu.h"
#include "../../../../../include/flswriter.h"
#include "duckdb/common/exception.hpp"
#include "duckdb/common/string_util.hpp"
#include "duckdb/function/table_function.hpp"
#include "type_mapping.hpp"

namespace duckdb {
namespace ext_fastlane {
namespace filter_text {

inline string Trim(const string &s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) ++a;
    while (b > a && isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

inline bool IsIdent(const string &s) {
    if (s.empty() || !(isalpha((unsigned char)s[0]) || s[0] == '_')) return false;
    for (char c : s)
        if (!(isalnum((unsigned char)c) || c == '_')) return false;
    return true;
}

struct Schema {
    std::vector<fls_column_info> cols;
    vector<string> names;
    vector<LogicalType> types;
    // exact name first, then case-insensitively (DuckDB's identifier matching)
    int Find(string name) const {
        if (name.size() >= 2 && name.front() == '"' && name.back() == '"') name = name.substr(1, name.size() - 2);
        for (size_t c = 0; c < names.size(); ++c)
            if (names[c] == name) return (int)c;
        const string low = StringUtil::Lower(name);
        for (size_t c = 0; c < names.size(); ++c)
            if (StringUtil::Lower(names[c]) == low) return (int)c;
        return -1;
    }
    // the table's columns, named and typed as read_fastlanes types them (footer only)
    void Load(fls_table *t) {
        const uint32_t n = fls_table_ncols(t);
        cols.resize(n);
        for (uint32_t c = 0; c < n; ++c) {
            fls_table_column(t, c, &cols[c]);
            types.push_back(TypeMapping::FastLanesToDuckDB(cols[c].type, cols[c].width, cols[c].scale));
            names.emplace_back(cols[c].name);
        }
    }
};

inline bool IsString(uint8_t t) { return t == FLS_VARCHAR || t == FLS_BLOB; }
inline bool IsFloat(uint8_t t) { return t == FLS_FLOAT || t == FLS_DOUBLE; }

struct Token {
    enum Kind { END, WORD, NUMBER, STRING, OP, PUNCT } kind = END;
    string text;   // WORD as written, NUMBER digits, STRING unescaped contents, OP the operator, PUNCT ( ) or ,
};

struct Lexer {
    const string &s;
    size_t pos = 0;
    string who;    // the table function the messages name
    explicit Lexer(const string &text, string who_p = "fastlanes_aggregate") : s(text), who(std::move(who_p)) {}
    Token Next() {
        while (pos < s.size() && isspace((unsigned char)s[pos])) ++pos;
        Token t;
        if (pos >= s.size()) return t;
        const char c = s[pos];
        if (isalpha((unsigned char)c) || c == '_') {
            const size_t a = pos;
            while (pos < s.size() && (isalnum((unsigned char)s[pos]) || s[pos] == '_')) ++pos;
            t.kind = Token::WORD;
            t.text = s.substr(a, pos - a);
            return t;
        }
        if (c == '"') {
            const size_t e = s.find('"', pos + 1);
            if (e == string::npos) throw BinderException(who + ": unterminated identifier in filter \"" + s + "\"");
            t.kind = Token::WORD;
            t.text = s.substr(pos, e + 1 - pos);
            pos = e + 1;
            return t;
        }
        if (c == '\'') {
            t.kind = Token::STRING;
            for (++pos;; ++pos) {
                if (pos >= s.size()) throw BinderException(who + ": unterminated string in filter \"" + s + "\"");
                if (s[pos] == '\'') {
                    if (pos + 1 < s.size() && s[pos + 1] == '\'') {
                        t.text += '\'';
                        ++pos;
                        continue;
                    }
                    ++pos;
                    return t;
                }
                t.text += s[pos];
            }
        }
        if (isdigit((unsigned char)c) || c == '.' || ((c == '-' || c == '+') && pos + 1 < s.size() &&
                                                      (isdigit((unsigned char)s[pos + 1]) || s[pos + 1] == '.'))) {
            const size_t a = pos++;
            while (pos < s.size() && (isalnum((unsigned char)s[pos]) || s[pos] == '.' ||
                                      ((s[pos] == '-' || s[pos] == '+') && (s[pos - 1] == 'e' || s[pos - 1] == 'E'))))
                ++pos;
            t.kind = Token::NUMBER;
            t.text = s.substr(a, pos - a);
            return t;
        }
        if (c == '(' || c == ')' || c == ',') {  // the brackets and commas of an IN list
            t.kind = Token::PUNCT;
            t.text = string(1, c);
            ++pos;
            return t;
        }
        for (const char *op : {"<>", "!=", "<=", ">=", "=", "<", ">"})
            if (s.compare(pos, strlen(op), op) == 0) {
                t.kind = Token::OP;
                t.text = op;
                pos += strlen(op);
                return t;
            }
        throw BinderException(who + ": cannot parse \"" + s.substr(pos, 1) + "\" in filter \"" + s + "\"");
    }
};

inline int64_t DaysFromCivil(int64_t y, unsigned m, unsigned d) {
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const unsigned yoe = (unsigned)(y - era * 400);
    const unsigned doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + (int64_t)doe - 719468;
}

inline bool AllDigits(const string &s) {
    if (s.empty()) return false;
    for (char c : s)
        if (!isdigit((unsigned char)c)) return false;
    return true;
}

// the literal of a comparison in the column's physical type (fls_predicate.value / str)
inline void SetLiteral(const Schema &sch, int col, Lexer &lex, Token lit, const string &filter, fls_predicate &p,
                       std::deque<string> &strs, const char *where = "filter") {
    const fls_column_info &ci = sch.cols[col];
    const string cname = sch.names[col];
    const string &who = lex.who;
    bool date_kw = false;
    if (lit.kind == Token::WORD && StringUtil::Lower(lit.text) == "date") {
        date_kw = true;
        lit = lex.Next();
        if (lit.kind != Token::STRING)
            throw BinderException(who + ": DATE needs a 'YYYY-MM-DD' string in " + where + " \"" + filter + "\"");
    }
    auto bad = [&](const char *want) {
        return BinderException(who + ": \"" + (lit.kind == Token::STRING ? "'" + lit.text + "'" : lit.text) +
                               "\" is not " + want + " for " + sch.types[col].ToString() + " column \"" + cname +
                               "\" in " + where + " \"" + filter + "\"");
    };
    if (lit.kind == Token::END || lit.kind == Token::OP || lit.kind == Token::PUNCT)
        throw BinderException(who + ": a literal is missing after column \"" + cname + "\" in " + where + " \"" +
                              filter + "\"");
    if (date_kw != (ci.type == FLS_DATE)) throw bad(ci.type == FLS_DATE ? "a DATE 'YYYY-MM-DD' literal" : "a literal");
    switch (ci.type) {
    case FLS_DATE: {
        int y = 0, n = 0;
        unsigned m = 0, d = 0;
        if (sscanf(lit.text.c_str(), "%d-%u-%u%n", &y, &m, &d, &n) != 3 || (size_t)n != lit.text.size() || m < 1 ||
            m > 12 || d < 1 || d > 31)
            throw bad("a DATE 'YYYY-MM-DD' literal");
        p.value = (uint64_t)DaysFromCivil(y, m, d);
        return;
    }
    case FLS_VARCHAR: case FLS_BLOB:
        if (lit.kind != Token::STRING) throw bad("a quoted string");
        strs.push_back(lit.text);
        p.str = strs.back().data();
        p.str_len = strs.back().size();
        return;
    case FLS_FLOAT: case FLS_DOUBLE: {
        if (lit.kind == Token::STRING) throw bad("a number");
        char *end = nullptr;
        const double d = std::strtod(lit.text.c_str(), &end);
        if (end == lit.text.c_str() || *end) throw bad("a number");
        if (ci.type == FLS_FLOAT) {
            const float f = (float)d;
            uint32_t b;
            memcpy(&b, &f, 4);
            p.value = b;
        } else {
            memcpy(&p.value, &d, 8);
        }
        return;
    }
    case FLS_BOOLEAN:
        if (lit.kind == Token::WORD && (StringUtil::Lower(lit.text) == "true" || StringUtil::Lower(lit.text) == "false")) {
            p.value = StringUtil::Lower(lit.text) == "true";
            return;
        }
        if (lit.kind != Token::NUMBER || (lit.text != "0" && lit.text != "1")) throw bad("true, false, 0 or 1");
        p.value = lit.text == "1";
        return;
    default: break;
    }
    // integers and DECIMAL: exact decimal text -> (scaled) integer
    if (lit.kind != Token::NUMBER) throw bad("a number");
    string t = lit.text;
    const bool neg = t[0] == '-';
    if (t[0] == '-' || t[0] == '+') t = t.substr(1);
    const size_t dot = t.find('.');
    string ip = dot == string::npos ? t : t.substr(0, dot), fp = dot == string::npos ? "" : t.substr(dot + 1);
    if ((!ip.empty() && !AllDigits(ip)) || (!fp.empty() && !AllDigits(fp)) || (ip.empty() && fp.empty()))
        throw bad("a number");
    while (!fp.empty() && fp.back() == '0') fp.pop_back();
    const unsigned scale = ci.type == FLS_DECIMAL ? ci.scale : 0;
    if (fp.size() > scale)
        throw bad(ci.type == FLS_DECIMAL ? "exactly representable (too many fractional digits)" : "an integer");
    fp.resize(scale, '0');
    const string digits = ip + fp;
    const bool is_unsigned = ci.type >= FLS_UINT8 && ci.type <= FLS_UINT64;
    unsigned __int128 v = 0;
    for (char c : digits) {
        v = v * 10 + (unsigned)(c - '0');
        if (v > ((unsigned __int128)1 << 64)) throw bad("in range");
    }
    if (is_unsigned) {
        if ((neg && v != 0) || v > UINT64_MAX) throw bad("in range");
        p.value = (uint64_t)v;
    } else {
        if (v > ((unsigned __int128)1 << 63) - (neg ? 0 : 1)) throw bad("in range");
        p.value = neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    }
}

// The key sets a filter's IN lists became (fls_keyset_create): freed with the
// bind data that owns the predicates.
struct KeySets {
    std::vector<fls_keyset *> sets;
    KeySets() = default;
    KeySets(const KeySets &) = delete;
    KeySets &operator=(const KeySets &) = delete;
    ~KeySets() {
        for (fls_keyset *s : sets) fls_keyset_free(s);
    }
};

// `column [NOT] IN (literal, ...)`, the lexer past IN.  On an integer-like
// column (everything but VARCHAR / BLOB / FLOAT / DOUBLE) the list becomes one
// key-set term; on the others IN becomes EQ terms of one clause and NOT IN NE
// terms of a clause each.  SQL's NULL rules: a NULL in an IN list is ignored
// (a list of nothing else matches no row), a NULL in a NOT IN list leaves no
// row (FLS_CMP_FALSE).
inline void ParseInList(const Schema &sch, int c, bool negate, Lexer &lex, const string &filter, uint32_t &clause,
                        std::vector<fls_predicate> &preds, std::deque<string> &strs, fls_connection *conn,
                        KeySets *sets) {
    const string &who = lex.who;
    const string what = negate ? "NOT IN" : "IN";
    Token t = lex.Next();
    if (t.kind != Token::PUNCT || t.text != "(")
        throw BinderException(who + ": \"(\" is expected after " + what + " in filter \"" + filter + "\"");
    std::vector<fls_predicate> lits;
    bool has_null = false;
    t = lex.Next();
    if (t.kind == Token::PUNCT && t.text == ")")
        throw BinderException(who + ": the " + what + " list of column \"" + sch.names[c] + "\" is empty in filter \"" +
                              filter + "\"");
    for (;;) {
        if (t.kind == Token::END)
            throw BinderException(who + ": \")\" is missing after the " + what + " list of column \"" + sch.names[c] +
                                  "\" in filter \"" + filter + "\"");
        if (t.kind == Token::WORD && StringUtil::Lower(t.text) == "null") {
            has_null = true;
        } else {
            fls_predicate p;
            memset(&p, 0, sizeof(p));
            p.col = (uint32_t)c;
            SetLiteral(sch, c, lex, t, filter, p, strs);
            lits.push_back(p);
        }
        t = lex.Next();
        if (t.kind == Token::PUNCT && t.text == ")") break;
        if (t.kind == Token::END)
            throw BinderException(who + ": \")\" is missing after the " + what + " list of column \"" + sch.names[c] +
                                  "\" in filter \"" + filter + "\"");
        if (t.kind != Token::PUNCT || t.text != ",")
            throw BinderException(who + ": \",\" or \")\" is expected at \"" + t.text + "\" in the " + what +
                                  " list of filter \"" + filter + "\"");
        t = lex.Next();
    }
    fls_predicate p;
    memset(&p, 0, sizeof(p));
    p.col = (uint32_t)c;
    if ((negate && has_null) || lits.empty()) {
        p.clause = clause++;
        p.op = FLS_CMP_FALSE;
        preds.push_back(p);
        return;
    }
    const uint8_t ty = sch.cols[c].type;
    if (IsString(ty) || IsFloat(ty)) {
        for (fls_predicate &l : lits) {
            l.op = negate ? FLS_CMP_NE : FLS_CMP_EQ;
            l.clause = negate ? clause++ : clause;
            preds.push_back(l);
        }
        if (!negate) ++clause;
        return;
    }
    std::vector<uint64_t> keys;
    for (const fls_predicate &l : lits) keys.push_back(l.value);
    const bool is_unsigned = (ty >= FLS_UINT8 && ty <= FLS_UINT64) || ty == FLS_BOOLEAN;
    fls_keyset *set = nullptr;
    if (!conn || !sets ||
        fls_keyset_create(conn, keys.data(), keys.size(), is_unsigned ? FLS_KEYSET_UNSIGNED : FLS_KEYSET_SIGNED,
                          FLS_KEYSET_AUTO, &set) != 0)
        throw BinderException(who + ": cannot build the key set of the " + what + " list in filter \"" + filter +
                              "\": " + (conn && sets ? fls_last_error() : "no connection"));
    sets->sets.push_back(set);
    p.clause = clause++;
    p.op = negate ? FLS_CMP_NOT_IN_SET : FLS_CMP_IN_SET;
    p.value = (uint64_t)(uintptr_t)set;
    preds.push_back(p);
}

// `column [NOT] LIKE 'pattern' [ESCAPE 'c']`, the lexer past LIKE: one pattern
// term (FLS_CMP_LIKE / FLS_CMP_NOT_LIKE, the escape byte in `value`), a clause
// of its own.  LIKE NULL matches no row (FLS_CMP_FALSE).
inline void ParseLike(const Schema &sch, int c, bool negate, Lexer &lex, const string &filter, uint32_t &clause,
                      std::vector<fls_predicate> &preds, std::deque<string> &strs) {
    const string &who = lex.who;
    const string what = negate ? "NOT LIKE" : "LIKE";
    if (sch.cols[c].type != FLS_VARCHAR)
        throw BinderException(who + ": " + what + " needs a VARCHAR column, \"" + sch.names[c] + "\" is " +
                              sch.types[c].ToString() + " in filter \"" + filter + "\"");
    fls_predicate p;
    memset(&p, 0, sizeof(p));
    p.col = (uint32_t)c;
    p.clause = clause++;
    Token pat = lex.Next();
    if (pat.kind == Token::WORD && StringUtil::Lower(pat.text) == "null") {
        p.op = FLS_CMP_FALSE;
        preds.push_back(p);
        return;
    }
    if (pat.kind != Token::STRING)
        throw BinderException(who + ": a quoted pattern is expected after " + what + ", found \"" + pat.text +
                              "\" in filter \"" + filter + "\"");
    p.op = negate ? FLS_CMP_NOT_LIKE : FLS_CMP_LIKE;
    const size_t after = lex.pos;  // ESCAPE is optional: look one token ahead
    Token t = lex.Next();
    if (t.kind == Token::WORD && StringUtil::Lower(t.text) == "escape") {
        Token e = lex.Next();
        if (e.kind != Token::STRING || e.text.size() != 1 || e.text[0] == '\0')
            throw BinderException(who + ": ESCAPE needs a string of one byte, found \"" +
                                  (e.kind == Token::STRING ? "'" + e.text + "'" : e.text) + "\" in filter \"" + filter +
                                  "\"");
        p.value = (uint8_t)e.text[0];
        for (size_t i = 0; i < pat.text.size(); ++i)
            if ((uint8_t)pat.text[i] == p.value && ++i >= pat.text.size())
                throw BinderException(who + ": the pattern \"'" + pat.text + "'\" ends in its escape byte \"" + e.text +
                                      "\" in filter \"" + filter + "\"");
    } else {
        lex.pos = after;
    }
    strs.push_back(pat.text);
    p.str = strs.back().data();
    p.str_len = strs.back().size();
    preds.push_back(p);
}

// `column op column`: the pairs the engine compares (include/flsgpu.h) -- two
// signed or two unsigned integer columns of any widths, two DATE, two DECIMAL
// of at most 64 bits and one scale, FLOAT / DOUBLE in any mix.
inline void CheckColumnPair(const Schema &sch, int a, int b, const string &who, const string &filter) {
    const fls_column_info &ca = sch.cols[a], &cb = sch.cols[b];
    auto is_unsigned = [](uint8_t t) { return (t >= FLS_UINT8 && t <= FLS_UINT64) || t == FLS_BOOLEAN; };
    const char *why = nullptr;
    if (IsString(ca.type) || IsString(cb.type)) why = "strings are compared with constants only";
    else if (IsFloat(ca.type) != IsFloat(cb.type)) why = "an integer-like column against a float";
    else if ((ca.type == FLS_DATE) != (cb.type == FLS_DATE)) why = "a DATE column against a non-DATE column";
    else if ((ca.type == FLS_DECIMAL) != (cb.type == FLS_DECIMAL)) why = "a DECIMAL column against a non-DECIMAL column";
    else if (ca.type == FLS_DECIMAL && (ca.width > 18 || cb.width > 18)) why = "a DECIMAL wider than 64 bits";
    else if (ca.type == FLS_DECIMAL && ca.scale != cb.scale) why = "DECIMALs of different scale";
    else if (!IsFloat(ca.type) && is_unsigned(ca.type) != is_unsigned(cb.type)) why = "a signed column against an unsigned column";
    if (why)
        throw BinderException(who + ": cannot compare " + sch.types[a].ToString() + " column \"" + sch.names[a] +
                              "\" with " + sch.types[b].ToString() + " column \"" + sch.names[b] + "\" (" + why +
                              ") in filter \"" + filter + "\"");
}

// The filter's one OR group: alternative i is preds[ranges[i].first ..
// ranges[i].first + ranges[i].n), its clause numbers its own
// (fls_scan_filter_alternatives).
struct Alternatives {
    std::vector<fls_predicate> preds;
    std::vector<fls_filter_alternative> ranges;
};
constexpr size_t kMaxBranches = 8;  // the engine's planes per call

// One term, its first token (the column) read already: its predicates --
// several for an IN list on a VARCHAR / FLOAT / DOUBLE column -- onto preds.
inline void ParseTerm(const Schema &sch, Lexer &lex, const Token &col, const string &filter, uint32_t &clause,
                      std::vector<fls_predicate> &preds, std::deque<string> &strs, fls_connection *conn, KeySets *sets) {
    const string &who = lex.who;
    if (col.kind != Token::WORD)
        throw BinderException(who + ": a column name is expected at \"" + col.text + "\" in filter \"" + filter + "\"");
    const int c = sch.Find(col.text);
    if (c < 0) throw BinderException(who + ": column \"" + col.text + "\" of filter \"" + filter + "\" not found");
    fls_predicate p;
    memset(&p, 0, sizeof(p));
    p.col = (uint32_t)c;
    Token op = lex.Next();
    bool in_list = op.kind == Token::WORD && StringUtil::Lower(op.text) == "in", negate = false;
    bool like = op.kind == Token::WORD && StringUtil::Lower(op.text) == "like";
    if (op.kind == Token::WORD && StringUtil::Lower(op.text) == "not") {
        Token t = lex.Next();
        const string low = t.kind == Token::WORD ? StringUtil::Lower(t.text) : "";
        if (low != "in" && low != "like")
            throw BinderException(who + ": NOT IN or NOT LIKE is expected after \"" + col.text + "\" in filter \"" +
                                  filter + "\"");
        negate = true;
        (low == "in" ? in_list : like) = true;
    }
    if (in_list || like) {
        if (like) ParseLike(sch, c, negate, lex, filter, clause, preds, strs);
        else ParseInList(sch, c, negate, lex, filter, clause, preds, strs, conn, sets);
        return;
    }
    p.clause = clause++;
    if (op.kind == Token::WORD && StringUtil::Lower(op.text) == "is") {
        Token t = lex.Next();
        bool is_not = false;
        if (t.kind == Token::WORD && StringUtil::Lower(t.text) == "not") {
            is_not = true;
            t = lex.Next();
        }
        if (t.kind != Token::WORD || StringUtil::Lower(t.text) != "null")
            throw BinderException(who + ": IS [NOT] NULL is expected after \"" + col.text + "\" in filter \"" + filter +
                                  "\"");
        p.op = is_not ? FLS_CMP_IS_NOT_NULL : FLS_CMP_IS_NULL;
    } else if (op.kind == Token::OP) {
        p.op = op.text == "="                        ? FLS_CMP_EQ
               : (op.text == "!=" || op.text == "<>") ? FLS_CMP_NE
               : op.text == "<"                      ? FLS_CMP_LT
               : op.text == "<="                     ? FLS_CMP_LE
               : op.text == ">"                      ? FLS_CMP_GT
                                                     : FLS_CMP_GE;
        // the right side: a column when it is an identifier the schema resolves and
        // neither NULL nor the start of a typed literal (DATE '...'); else a literal
        Token rhs = lex.Next();
        const string low = rhs.kind == Token::WORD ? StringUtil::Lower(rhs.text) : "";
        bool typed = false;
        if (low == "date") {
            const size_t after = lex.pos;
            typed = lex.Next().kind == Token::STRING;
            lex.pos = after;
        }
        const bool word = rhs.kind == Token::WORD && low != "null" && !typed;
        const int c2 = word ? sch.Find(rhs.text) : -1;
        if (c2 >= 0) {
            CheckColumnPair(sch, c, c2, who, filter);
            p.op = (uint8_t)(FLS_CMP_COL_EQ + p.op);
            p.value = (uint64_t)c2;
        } else if (word && low != "date") {
            // a word that names no column is still a literal where it was one before (nan, inf,
            // infinity on a FLOAT / DOUBLE column, true / false on a BOOLEAN one); only a word
            // the literal parser refuses as well is reported as an unknown column
            try {
                SetLiteral(sch, c, lex, rhs, filter, p, strs);
            } catch (const BinderException &) {
                throw BinderException(who + ": column \"" + rhs.text + "\" on the right of \"" + col.text + " " +
                                      op.text + "\" in filter \"" + filter + "\" not found");
            }
        } else {
            SetLiteral(sch, c, lex, rhs, filter, p, strs);
        }
    } else {
        throw BinderException(who + ": a comparison or IS [NOT] NULL is expected after \"" + col.text +
                              "\" in filter \"" + filter + "\"");
    }
    preds.push_back(p);
}

// filter := item (AND item)*
// item   := term | '(' branch (OR branch)+ ')'
// branch := term | '(' term (AND term)* ')'
// The AND-ed terms go to preds; the OR group (at most one, 2 to 8 branches)
// to alts, a branch an alternative.  alts == NULL (the condition text of an
// aggregate's FILTER (WHERE ...)): no OR group.
inline void ParseFilter(const Schema &sch, const string &filter, std::vector<fls_predicate> &preds,
                        std::deque<string> &strs, const string &who = "fastlanes_aggregate",
                        fls_connection *conn = nullptr, KeySets *sets = nullptr, Alternatives *alts = nullptr) {
    if (Trim(filter).empty()) return;
    Lexer lex(filter, who);
    uint32_t clause = 0;
    auto open_paren = [](const Token &t) { return t.kind == Token::PUNCT && t.text == "("; };
    auto close_paren = [](const Token &t) { return t.kind == Token::PUNCT && t.text == ")"; };
    auto is_word = [](const Token &t, const char *w) { return t.kind == Token::WORD && StringUtil::Lower(t.text) == w; };
    auto shown = [](const Token &t) { return t.kind == Token::END ? string("end of text") : t.text; };
    for (;;) {
        const size_t at = lex.pos;
        Token first = lex.Next();
        if (open_paren(first)) {
            const string rest = Trim(filter.substr(at));
            if (!alts)
                throw BinderException(who + ": an OR group is not supported in a FILTER (WHERE ...) condition, found \"" +
                                      rest + "\" in \"" + filter + "\"");
            if (!alts->ranges.empty())
                throw BinderException(who + ": a second OR group \"" + rest + "\" in filter \"" + filter +
                                      "\" (one per filter)");
            for (;;) {  // a branch
                if (alts->ranges.size() == kMaxBranches)
                    throw BinderException(who + ": more than " + std::to_string(kMaxBranches) +
                                          " branches in the OR group of filter \"" + filter + "\"");
                fls_filter_alternative r;
                r.first = (uint32_t)alts->preds.size();
                uint32_t local = 0;  // clause numbers are the alternative's own
                const size_t bat = lex.pos;
                Token t = lex.Next();
                if (open_paren(t)) {
                    for (;;) {
                        const size_t tat = lex.pos;
                        t = lex.Next();
                        if (open_paren(t))
                            throw BinderException(who + ": a parenthesis nested deeper than a branch at \"" +
                                                  Trim(filter.substr(tat)) + "\" in filter \"" + filter + "\"");
                        ParseTerm(sch, lex, t, filter, local, alts->preds, strs, conn, sets);
                        t = lex.Next();
                        if (close_paren(t)) break;
                        if (!is_word(t, "and"))
                            throw BinderException(who + ": AND or \")\" is expected in the branch \"" +
                                                  Trim(filter.substr(bat, lex.pos - bat)) + "\", found \"" + shown(t) +
                                                  "\" in filter \"" + filter + "\"");
                    }
                } else {
                    ParseTerm(sch, lex, t, filter, local, alts->preds, strs, conn, sets);
                }
                r.n = (uint32_t)alts->preds.size() - r.first;
                alts->ranges.push_back(r);
                t = lex.Next();
                if (close_paren(t)) break;
                if (!is_word(t, "or"))
                    throw BinderException(who + ": OR or \")\" is expected after the branch \"" +
                                          Trim(filter.substr(bat, lex.pos - bat)) + "\", found \"" + shown(t) +
                                          "\" (a branch of several terms takes its own parentheses) in filter \"" +
                                          filter + "\"");
            }
            if (alts->ranges.size() < 2)
                throw BinderException(who + ": \"(\" opens an OR group of 2 to 8 branches, \"" +
                                      Trim(filter.substr(at, lex.pos - at)) + "\" holds no OR in filter \"" + filter + "\"");
        } else {
            ParseTerm(sch, lex, first, filter, clause, preds, strs, conn, sets);
        }
        Token next = lex.Next();
        if (next.kind == Token::END) return;
        if (!is_word(next, "and"))
            throw BinderException(who + ": only AND joins filter terms, found \"" + next.text + "\" in filter \"" + filter +
                                  "\"");
    }
}

}  // namespace filter_text
}  // namespace ext_fastlane
}  // namespace duckdb
