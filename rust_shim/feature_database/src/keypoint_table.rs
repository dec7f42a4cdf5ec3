//! The id-taking access paths of the reference's `KeypointDatabase` trait (feature_database/src/keypointdb.rs) on the GPU-resident
//! keypoint table: `read_keypoint_from_id` (keypointdb.rs:28-36), `delete_keypoint` (keypointdb.rs:92-97), and the deletes by image, level
//! of detail and region that replacing imagery needs. The table is filled by the preprocessor side (`apds_mosaic_tiles_to_db`,
//! `apds_db_insert_dev`); `handle()` is what those calls and `FramePipeline::new_table` take. Ids behave like the SERIAL column of the
//! reference: never reused, unchanged by deletes, continued by inserts. A delete is a writer like an insert: one thread per table, never
//! while a view's select is in flight or a pipeline holds the table. NOT compiled in the build container (no Rust toolchain there).
use apds_sys::apds_keypoint;
use std::ffi::CStr;
use std::os::raw::c_void;
use std::ptr;

pub const APDS_ERR_OUT_OF_RANGE: i32 = -211;

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

pub struct KeypointTable {
    db: *mut c_void,
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

    pub fn handle(&self) -> *mut c_void {
        self.db
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
