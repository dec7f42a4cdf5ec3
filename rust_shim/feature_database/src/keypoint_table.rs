//! The id-taking access paths of the reference's `KeypointDatabase` trait (feature_database/src/keypointdb.rs) on the GPU-resident
//! keypoint table: `read_keypoint_from_id` (keypointdb.rs:28-36), `delete_keypoint` (keypointdb.rs:92-97), and the deletes by image, level
//! of detail and region that replacing imagery needs. The table is filled by the preprocessor side (`apds_mosaic_tiles_to_db`,
//! `apds_db_insert_dev`); `handle()` is what those calls and `FramePipeline::new_table` take. Ids behave like the SERIAL column of the
//! reference: never reused, unchanged by deletes, continued by inserts. A delete is a writer like an insert: one thread per table, never
//! while a view's select is in flight or a pipeline holds the table. A table is a byte table (`create`: 61-byte M-LDB descriptors) or a
//! float table (`new_float`: rows of 64 floats for the L2 matcher); the `_float` methods, `l2_knn_match` and `TableView::l2_train` are the
//! float table's. NOT compiled in the build container (no Rust toolchain there).
use apds_sys::apds_keypoint;
use std::ffi::CStr;
use std::marker::PhantomData;
use std::os::raw::c_void;
use std::ptr;

pub const APDS_ERR_OUT_OF_RANGE: i32 = -211;
pub const APDS_AKAZE_DESCRIPTOR_KAZE: i32 = 3;
pub const APDS_L2_EXACT: i32 = 0;
pub const APDS_L2_SCREEN: i32 = 1;
/// floats per row of a float table (APDS_DESC_FLOAT_DIM)
pub const FLOAT_DIM: usize = 64;

fn err(rc: i32) -> String {
    format!("apds error {}: {}", rc, unsafe { CStr::from_ptr(apds_sys::apds_last_error()) }.to_string_lossy())
}

/// What `models::Keypoint` holds (models.rs:27-41) for one row.
pub struct KeypointRow {
    pub id: i32,
    pub keypoint: apds_keypoint,
    pub descriptor: [u8; 61],
    pub image_id: i32,
    /// the row's current position in the table (trainIdx of a whole-table pipeline)
    pub row: i64,
}

/// The same for a row of a float table (`KeypointTable::new_float`): the descriptor is the row's 64 floats.
pub struct KeypointRowFloat {
    pub id: i32,
    pub keypoint: apds_keypoint,
    pub descriptor: [f32; FLOAT_DIM],
    pub image_id: i32,
    /// the row's current position in the table; -1 in the rows a selection returns
    pub row: i64,
}

pub struct KeypointTable {
    db: *mut c_void,
}

/// A view of a table (`KeypointTable::view`): the per-frame read of keypointdb.rs:50-90, left on the device. On a float table the view
/// also owns the L2 train side of its selection, written by the select's own gather.
pub struct TableView<'t> {
    view: *mut c_void,
    _table: PhantomData<&'t KeypointTable>,
}

impl TableView<'_> {
    pub fn handle(&self) -> *mut c_void {
        self.view
    }

    /// `apds_db_view_select` on `stream` (null: the calling thread's own): the rows now in the view. Mode 0 image id, 1 level of detail,
    /// 2 level of detail and bounding box.
    #[allow(clippy::too_many_arguments)]
    pub fn select(&self, mode: i32, value: i32, x_start: f32, y_start: f32, x_end: f32, y_end: f32, with_xyz: bool, stream: *mut c_void) -> Result<i32, String> {
        let mut n = 0i32;
        let rc = unsafe { apds_sys::apds_db_view_select(self.view, mode, value, x_start, y_start, x_end, y_end, with_xyz as i32, stream, &mut n) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(n)
    }

    /// A float table's view: the train set over the last selection, for `l2_train_top2`. Borrowed from the view: valid while the view
    /// lives, following every select, never to be destroyed by the caller. `Err` on a view of a byte table.
    pub fn l2_train(&self) -> Result<*mut c_void, String> {
        let mut set = ptr::null_mut();
        let rc = unsafe { apds_sys::apds_db_view_l2_train(self.view, &mut set) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(set)
    }

    /// The two nearest rows of the view's selection for `n_query` device rows of 64 floats, as keys (f32 bits of d^2 << 32 | position in the
    /// view) into `out_keys_dev` (n_query x 2 u64 on the device), on `stream`. `mode`: APDS_L2_SCREEN or APDS_L2_EXACT; returns the mode
    /// that ran (a selection of fewer than two rows is served by the exact kernel).
    pub fn l2_train_top2(&self, query_f32_dev: *const c_void, n_query: i32, mode: i32, out_keys_dev: *mut c_void, stream: *mut c_void) -> Result<i32, String> {
        let set = self.l2_train()?;
        let mut used = APDS_L2_EXACT;
        let rc = unsafe { apds_sys::apds_dev_l2_train_top2(set, query_f32_dev, n_query, mode, out_keys_dev, stream, &mut used, ptr::null_mut()) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(used)
    }
}

impl Drop for TableView<'_> {
    fn drop(&mut self) {
        unsafe {
            apds_sys::apds_db_view_destroy(self.view);
        }
    }
}

impl KeypointTable {
    pub fn create(gpu: i32, capacity: i64) -> Result<Self, String> {
        let mut db = ptr::null_mut();
        let mut rc = unsafe { apds_sys::apds_set_device(gpu) };
        if rc == 0 {
            rc = unsafe { apds_sys::apds_db_create(&mut db, capacity) };
        }
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(KeypointTable { db })
    }

    /// A table whose descriptor column is 64 x f32 (the M-SURF rows of `apds_akaze_extract_float`, the L2 matcher's input). Every method
    /// of this type serves both kinds except the typed ones: the `_float` methods below are a float table's, their byte-typed twins a
    /// byte table's, and a call of the wrong kind is an `Err` (APDS_ERR_BAD_ARG) that leaves the table unchanged.
    pub fn new_float(gpu: i32, capacity: i64) -> Result<Self, String> {
        let mut db = ptr::null_mut();
        let mut rc = unsafe { apds_sys::apds_set_device(gpu) };
        if rc == 0 {
            rc = unsafe { apds_sys::apds_db_create_float(&mut db, capacity) };
        }
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(KeypointTable { db })
    }

    pub fn handle(&self) -> *mut c_void {
        self.db
    }

    /// (is_float, bytes of a descriptor row on the device: 64 or 256)
    pub fn kind(&self) -> Result<(bool, i32), String> {
        let (mut descriptor, mut row_bytes) = (0i32, 0i32);
        let rc = unsafe { apds_sys::apds_db_info(self.db, &mut descriptor, &mut row_bytes) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok((descriptor == APDS_AKAZE_DESCRIPTOR_KAZE, row_bytes))
    }

    /// preprocessor/src/main.rs:296-324 on a float table: every keypoint of one tile, `descriptors` = 64 floats per keypoint.
    #[allow(clippy::too_many_arguments)]
    pub fn insert_image_float(&self, keypoints: &[apds_keypoint], descriptors: &[f32], image_id: i32, level_of_detail: i32, column: u64, row: u64,
                              tile_w: u64, tile_h: u64) -> Result<(), String> {
        if descriptors.len() != keypoints.len() * FLOAT_DIM {
            return Err(format!("{} keypoints need {} floats, got {}", keypoints.len(), keypoints.len() * FLOAT_DIM, descriptors.len()));
        }
        let rc = unsafe {
            apds_sys::apds_db_insert_image_float(self.db, keypoints.as_ptr(), descriptors.as_ptr(), keypoints.len() as i32, image_id, level_of_detail, column, row,
                                                 tile_w, tile_h)
        };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(())
    }

    /// keypointdb.rs:38-90 on a float table: `apds_db_select` (mode 0 image id, 1 level of detail, 2 level of detail and bounding box), then
    /// the host copy of the selection: best response first, at most 262143 rows.
    pub fn select_float(&self, mode: i32, value: i32, x_start: f32, y_start: f32, x_end: f32, y_end: f32) -> Result<Vec<KeypointRowFloat>, String> {
        let mut n = 0i32;
        let rc = unsafe { apds_sys::apds_db_select(self.db, mode, value, x_start, y_start, x_end, y_end, &mut n) };
        if rc != 0 {
            return Err(err(rc));
        }
        let m = n.max(0) as usize;
        let mut kps: Vec<apds_keypoint> = (0..m).map(|_| unsafe { std::mem::zeroed() }).collect();
        let (mut desc, mut ids, mut images) = (vec![0f32; m * FLOAT_DIM], vec![0i32; m], vec![0i32; m]);
        if m > 0 {
            let rc = unsafe { apds_sys::apds_db_view_download_float(self.db, kps.as_mut_ptr(), desc.as_mut_ptr(), ids.as_mut_ptr(), images.as_mut_ptr()) };
            if rc != 0 {
                return Err(err(rc));
            }
        }
        Ok((0..m)
            .map(|i| {
                let mut descriptor = [0f32; FLOAT_DIM];
                descriptor.copy_from_slice(&desc[i * FLOAT_DIM..(i + 1) * FLOAT_DIM]);
                KeypointRowFloat { id: ids[i], keypoint: kps[i], descriptor, image_id: images[i], row: -1 }
            })
            .collect())
    }

    /// BFMatcher(NORM_L2).knnMatch (k = 1 or 2) of `n_query` rows of 64 floats against the table's last selection (`select_float`), which
    /// stays on the device: (index into that selection or -1, distance or +inf) per query and neighbour.
    pub fn l2_knn_match(&self, query: &[f32], k: i32) -> Result<(Vec<i32>, Vec<f32>), String> {
        let nq = query.len() / FLOAT_DIM;
        if query.len() != nq * FLOAT_DIM || k < 1 {
            return Err("query: a whole number of rows of 64 floats; k >= 1".to_string());
        }
        let (mut idx, mut dist) = (vec![-1i32; nq * k as usize], vec![f32::INFINITY; nq * k as usize]);
        let rc = unsafe { apds_sys::apds_db_l2_knn_match(self.db, query.as_ptr(), nq as i32, k, idx.as_mut_ptr(), dist.as_mut_ptr()) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok((idx, dist))
    }

    /// `read_keypoint_from_id` on a float table.
    pub fn read_keypoint_from_id_float(&self, id: i32) -> Result<Option<KeypointRowFloat>, String> {
        let mut out = KeypointRowFloat { id, keypoint: unsafe { std::mem::zeroed() }, descriptor: [0.0; FLOAT_DIM], image_id: 0, row: -1 };
        let rc =
            unsafe { apds_sys::apds_db_read_keypoint_from_id_float(self.db, id, &mut out.keypoint, out.descriptor.as_mut_ptr(), &mut out.image_id, &mut out.row) };
        match rc {
            0 => Ok(Some(out)),
            APDS_ERR_OUT_OF_RANGE => Ok(None),
            _ => Err(err(rc)),
        }
    }

    /// A view of this table (keypointdb.rs:50-90 as a per-frame read; `capacity` <= 0: as many rows as a select can return). The view
    /// borrows the table: it cannot outlive it.
    pub fn view(&self, capacity: i32) -> Result<TableView<'_>, String> {
        let mut view = ptr::null_mut();
        let rc = unsafe { apds_sys::apds_db_view_create(self.db, capacity, &mut view) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(TableView { view, _table: PhantomData })
    }

    pub fn rows(&self) -> i64 {
        unsafe { apds_sys::apds_db_rows(self.db) }
    }

    /// keypointdb.rs:28-36; `Ok(None)` where the reference returns `Err(NotFound)`: the id was deleted or never given.
    pub fn read_keypoint_from_id(&self, id: i32) -> Result<Option<KeypointRow>, String> {
        let mut out = KeypointRow { id, keypoint: unsafe { std::mem::zeroed() }, descriptor: [0; 61], image_id: 0, row: -1 };
        let rc = unsafe { apds_sys::apds_db_read_keypoint_from_id(self.db, id, &mut out.keypoint, out.descriptor.as_mut_ptr(), &mut out.image_id, &mut out.row) };
        match rc {
            0 => Ok(Some(out)),
            APDS_ERR_OUT_OF_RANGE => Ok(None),
            _ => Err(err(rc)),
        }
    }

    /// keypointdb.rs:92-97: `Ok(())` whether or not the id existed.
    pub fn delete_keypoint(&self, id: i32) -> Result<(), String> {
        self.delete_keypoints(&[id]).map(|_| ())
    }

    /// The same for a list of ids in one compaction; unknown ids delete nothing, duplicates count once. Returns the rows deleted.
    pub fn delete_keypoints(&self, ids: &[i32]) -> Result<i64, String> {
        let mut n = 0i64;
        let rc = unsafe { apds_sys::apds_db_delete_ids(self.db, ids.as_ptr(), ids.len() as i32, &mut n) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(n)
    }

    fn delete_where(&self, mode: i32, value: i32, x_start: f32, y_start: f32, x_end: f32, y_end: f32) -> Result<i64, String> {
        let mut n = 0i64;
        let rc = unsafe { apds_sys::apds_db_delete_where(self.db, mode, value, x_start, y_start, x_end, y_end, &mut n) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(n)
    }

    /// Every row `read_keypoints_from_image_id` (keypointdb.rs:38-48) qualifies, without its row limit.
    pub fn delete_keypoints_from_image_id(&self, image_id: i32) -> Result<i64, String> {
        self.delete_where(0, image_id, 0.0, 0.0, 0.0, 0.0)
    }

    /// Every row `read_keypoints_from_lod` (keypointdb.rs:50-65) qualifies.
    pub fn delete_keypoints_from_lod(&self, level_of_detail: i32) -> Result<i64, String> {
        self.delete_where(1, level_of_detail, 0.0, 0.0, 0.0, 0.0)
    }

    /// Every row `read_keypoints_from_coordinates` (keypointdb.rs:67-90) qualifies: floor(start) <= v <= ceil(end).
    pub fn delete_keypoints_from_coordinates(&self, x_start: f32, y_start: f32, x_end: f32, y_end: f32, level_of_detail: i32) -> Result<i64, String> {
        self.delete_where(2, level_of_detail, x_start, y_start, x_end, y_end)
    }

    /// The id of every row, by row: index it with a match's trainIdx (whole-table pipeline) or a view's row ids.
    pub fn ids(&self) -> Result<Vec<i32>, String> {
        let mut host = vec![0i32; self.rows().max(0) as usize];
        if host.is_empty() {
            return Ok(host);
        }
        let mut ids_dev = ptr::null_mut();
        let mut rc = unsafe { apds_sys::apds_db_ids(self.db, &mut ids_dev) };
        if rc == 0 {
            rc = unsafe { apds_sys::apds_dev_download(host.as_mut_ptr() as *mut c_void, ids_dev, host.len() * 4, ptr::null_mut()) };
        }
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(host)
    }
}

impl Drop for KeypointTable {
    fn drop(&mut self) {
        unsafe {
            apds_sys::apds_db_destroy(self.db);
        }
    }
}
