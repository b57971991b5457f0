//===----------------------------------------------------------------------===//
//                         DuckDB - fastlane (MI355X)
//
// table_function/fastlanes_topn.hpp -- `fastlanes_topn(path, order_by, k[,
// filter[, columns]])`: ORDER BY one column [DESC] LIMIT k selected on the GPU
// under a pushed-down filter (fls_topn); at most 1024 rows.  Not in the
// reference, which delivers every decoded row to DuckDB.
//===----------------------------------------------------------------------===//
#pragma once

#include "duckdb/function/table_function.hpp"

namespace duckdb {
namespace ext_fastlane {

void RegisterFastlanesTopn(DatabaseInstance &db);

}  // namespace ext_fastlane
}  // namespace duckdb
