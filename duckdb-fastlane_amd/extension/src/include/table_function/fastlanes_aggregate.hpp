//===----------------------------------------------------------------------===//
//                         DuckDB - fastlane (MI355X)
//
// table_function/fastlanes_aggregate.hpp -- `fastlanes_aggregate(path,
// aggregates[, filter])`: ungrouped COUNT / SUM / MIN / MAX evaluated on the
// GPU under a pushed-down filter (fls_aggregate); one row.  Not in the
// reference, which delivers every decoded row to DuckDB.
//===----------------------------------------------------------------------===//
#pragma once

#include "duckdb/function/table_function.hpp"

namespace duckdb {
namespace ext_fastlane {

void RegisterFastlanesAggregate(DatabaseInstance &db);

}  // namespace ext_fastlane
}  // namespace duckdb
